"""The launcher of the multi-rank checks (tests/mr_gpu_*.py under torch.distributed.run), shared by every test that starts one."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUB = os.path.join(ROOT, "tests", "rccl_stub", "librccl_stub.so")
_RDZV_ERRORS = ("address already in use", "EADDRINUSE", "RendezvousConnectionError", "RendezvousTimeoutError", "DistNetworkError",
                "failed to bind", "The server socket has failed")


def run_check(args, timeout, env=None, transport="staged"):
    """Launch tests/mr_gpu_check.py under torch.distributed.run.  torchrun itself binds a free rendezvous port
    (--standalone), so there is no window between choosing and binding it.  The launch is repeated ONCE, and only
    when there is no verdict AND stderr names a rendezvous / bind error; a run that ends without a verdict for any
    other reason (a rank that aborted or faulted) fails with its output, and a FAILED verdict is never retried."""
    env = dict(os.environ, **(env or {}))
    if transport == "native":
        if not os.path.exists(STUB):
            subprocess.check_call(["make", "-s", "-C", os.path.dirname(STUB)])
        env["POP_RCCL_LIB"] = STUB
        args = args + ["--transport", "native"]
    out = None
    for attempt in range(2):
        cmd = [sys.executable, "-m", "torch.distributed.run", "--standalone", "--local-addr", "127.0.0.1", "--nnodes=1"] + args
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, env=env)
        if "MR_GPU_CHECK" in out.stdout or not any(e in out.stderr for e in _RDZV_ERRORS):
            break
    assert "MR_GPU_CHECK OK" in out.stdout, out.stdout[-6000:] + out.stderr[-3000:]
    return out.stdout
