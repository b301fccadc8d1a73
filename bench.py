#!/usr/bin/env python3
"""bench.py -- POP2 dynamics hot path on N MI355X GPUs of one node (one process per GPU).

  python bench.py --gpus 1 --steps K --warmup W
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N --steps K --warmup W
  python bench.py --gpus N ...        (no launcher: starts the line above itself as a child process and relays its JSON line)

A "step" is one full model time step (step_mod.F90 `step`: dhdt -> baroclinic_driver ->
barotropic_driver -> baroclinic_correct_adjust -> halo updates / time-level update) on synthetic
bathymetry and forcing, all state resident in HBM before the timed region.  The headline value is
simulated years per day (SYPD = 86400 / (t_step * step_calls_per_day * 365); step_calls_per_day = steps_per_day
plus the averaging half-steps of time_mix_opt = 'avgfit': 319 for tx0.1v3, not 300); ms_per_step
is the step wall time.  N > 1 shards the SAME global domain by blocks (strong scaling) with halo
exchange and the solver's block-sum all-reduce on RCCL (torch.distributed backend "nccl").

Rank 0 prints ONE JSON line.  A plain run sets up, warms up, times the steps and prints it; with --full
the line also carries `roofline` (every phase kernel HIP-event timed in runs of its own after the timed
steps) and, at N = 1, `kpp_deep_state` (tx0.1v3: a second state, stepped after the timed region) and
`cpu_baseline` (the CPU oracle = restated reference algorithm, timed on the host's cores).
--dump-outputs DIR (N = 1) writes the state the last timed step left as DIR/<name>.npy (see dump_outputs).
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

# algorithmic fp64 words per 3-D cell per launch of each phase kernel
PHASE_WORDS = {
    # phase: (const vmix, rich vmix, kpp)
    "vmix": (4, 7, 9),
    "tracer_rhs": (9, 9, 12),
    "impvmixt": (7, 7, 8),
    "state": (3, 3, 3),
    "momentum_rhs": (10, 10, 10),
    "impvmixu": (7, 7, 7),
    "correct": (6, 6, 7),
    "add_btrop": (4, 4, 4),
}
HBM_PEAK_GBS = 8000.0    # MI355X HBM3E spec peak (MI355X_MICROARCH.md); ~6300 GB/s achievable


def workload_config(name, nranks, block_rows=0):
    from popcfg import named_config
    cfg = named_config(name)
    if block_rows:
        if cfg.ny_global % block_rows:
            raise SystemExit("ny_global=%d not divisible by --block-rows %d" % (cfg.ny_global, block_rows))
        cfg.block_size_y = block_rows
        cfg.distribution_type = 1
    elif nranks > 1:
        # shard by j-bands.  Large grids: more bands than ranks (16, or 4 per rank) handed out as contiguous runs of equal
        # OCEAN columns (distribution_type = 1, the reference's load-balanced distributions): with land elimination a rank's
        # time follows its ocean columns, and equal bands of tx0.1v3's synthetic topography differ by 1.46 x at 8 ranks
        # (1.16 x with 75-row bands, 1.06 x at 4 ranks, 1.00 x at 2).  Small grids: one band per rank.
        if cfg.ny_global % nranks:
            raise SystemExit("ny_global=%d not divisible by %d ranks" % (cfg.ny_global, nranks))
        cfg.block_size_y = cfg.ny_global // nranks
        bands = max(16, 4 * nranks)
        # (two ranks keep one band each: 1.155 x against 1.00 x balanced, but several blocks per rank cost ~7% themselves --
        # measured on one GPU, tx0.1v3 as 8 blocks: 124.8 ms against 116.1)
        if nranks >= 4 and cfg.ny_global % bands == 0 and cfg.ny_global // bands >= 64:
            cfg.block_size_y = cfg.ny_global // bands
            cfg.distribution_type = 1
    return cfg


class TorchComm:
    """RCCL transport for the library's halo messages and block-sum all-reduce.  The library packs
    into / unpacks from torch-owned device buffers; everything runs on torch's current stream."""

    def __init__(self, pkg, model, rank, nranks, staged=False):
        # staged=True: CPU-staged transport over a gloo group (tests on one GPU); default: RCCL
        import torch
        import torch.distributed as dist
        self.torch, self.dist = torch, dist
        n = int(model.L.pop_comm_buffer_doubles(model.h))
        dev = torch.device("cuda", torch.cuda.current_device())
        self.send = torch.zeros(n, dtype=torch.float64, device=dev)
        self.recv = torch.zeros(n, dtype=torch.float64, device=dev)
        nred = max(int(model.L.pop_reduce_buffer_doubles(model.h)), 8)
        self.red = torch.zeros(nred, dtype=torch.float64, device=dev)

        def xchg(user, nmsg, peer, soff, scnt, roff, rcnt):
            try:
                ops, back = [], []
                if staged:
                    torch.cuda.synchronize()
                for i in range(nmsg):
                    if rcnt[i]:
                        dst = self.recv[roff[i]:roff[i] + rcnt[i]]
                        buf = torch.empty(rcnt[i], dtype=torch.float64) if staged else dst
                        if staged:
                            back.append((dst, buf))
                        ops.append(dist.P2POp(dist.irecv, buf, peer[i]))
                    if scnt[i]:
                        src = self.send[soff[i]:soff[i] + scnt[i]]
                        ops.append(dist.P2POp(dist.isend, src.cpu() if staged else src, peer[i]))
                if ops:
                    for r in dist.batch_isend_irecv(ops):
                        r.wait()
                for dst, buf in back:
                    dst.copy_(buf)
                return 0
            except Exception as e:  # noqa: BLE001
                print("exchange failed:", e, file=sys.stderr)
                return 1

        def allred(user, off, cnt):
            try:
                if staged:
                    torch.cuda.synchronize()
                    h = self.red[off:off + cnt].cpu()
                    dist.all_reduce(h)
                    self.red[off:off + cnt].copy_(h)
                else:
                    dist.all_reduce(self.red[off:off + cnt])
                return 0
            except Exception as e:  # noqa: BLE001
                print("allreduce failed:", e, file=sys.stderr)
                return 1

        self._x, self._a = pkg.XCHG_FN(xchg), pkg.ALLRED_FN(allred)
        # a dedicated non-default stream shared by the library's kernels and torch's collectives
        # (graph capture is not allowed on the legacy default stream)
        self.stream = torch.cuda.Stream()
        torch.cuda.set_stream(self.stream)
        model._chk(model.L.pop_set_stream(model.h, C.c_void_p(self.stream.cuda_stream)))
        model._chk(model.L.pop_set_reduce_buffer(model.h, C.c_void_p(self.red.data_ptr()), nred))
        model._chk(model.L.pop_set_comm(model.h, C.c_void_p(self.send.data_ptr()), C.c_void_p(self.recv.data_ptr()),
                                        C.c_void_p(self.red.data_ptr()), n, self._x, self._a, None))


_CPU_CHILD = r"""
import sys, time
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
from popcfg import PopConfig
from orclib import Oracle
cfg = PopConfig.from_buffer_copy(bytes.fromhex(sys.argv[2]))
budget, nmax = float(sys.argv[3]), int(sys.argv[4])
o = Oracle(cfg)
o.step()                      # forward-Euler first step excluded (BASELINE.md procedure)
print("READY", flush=True)
sys.stdin.readline()          # all processes start the timed steps together
t0 = time.time(); n = 0
while True:
    o.step(); n += 1
    if time.time() - t0 > budget or n >= nmax:
        break
print("DONE %d %.6f" % (n, time.time() - t0), flush=True)
"""


def cpu_baseline(cfg, budget_s=20.0, use_o3=True):
    """Time the CPU oracle on the host cores for a bounded number of steps.  C = min(cores, 16) processes (the
    oracle is a scalar port; POP_BENCH_CPU_CORES overrides) each step an equal sub-domain with the workload's
    options (same km, physics, time step) at the same time -- the block decomposition an MPI run of the reference
    would use, without its messages.  The sub-domain is at most 10 M cells and at most 1/C of the domain; the step
    time of the full domain is the slowest process's time per step divided by the fraction of the columns the C
    samples cover (the oracle's cost is linear in columns).  Children are started as separate programs (this
    process has initialised the GPU and must not fork)."""
    import copy
    import subprocess
    cores = int(os.environ.get("POP_BENCH_CPU_CORES", min(os.cpu_count() or 1, 16)))
    ncol = cfg.nx_global * cfg.ny_global
    div = 1
    while div * div < cores or (cfg.nx_global // div) * (cfg.ny_global // div) * cfg.km > 10_000_000:
        div *= 2
    while cfg.nx_global % div or cfg.ny_global % div:
        div //= 2
    cores = min(cores, div * div)
    sample_cfg = copy.copy(cfg)
    sample_cfg.nx_global, sample_cfg.ny_global = cfg.nx_global // div, cfg.ny_global // div
    sample_cfg.block_size_x, sample_cfg.block_size_y = sample_cfg.nx_global, sample_cfg.ny_global
    scale = cores * (sample_cfg.nx_global * sample_cfg.ny_global) / float(ncol)
    env = dict(os.environ, OMP_NUM_THREADS="1")
    o3 = os.path.join(ROOT, "oracle", "libpop_oracle_O3.so")      # -O3 -march=x86-64-v3 build of the oracle (timing only)
    if use_o3 and os.path.exists(o3):
        env["POP_ORACLE_LIB"] = o3
    procs = [subprocess.Popen([sys.executable, "-c", _CPU_CHILD, ROOT, bytes(sample_cfg).hex(), str(budget_s), "10"],
                              stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, env=env) for _ in range(cores)]
    try:
        for p in procs:
            if p.stdout.readline().strip() != "READY":
                raise RuntimeError("cpu baseline child failed to start")
        for p in procs:
            p.stdin.write("go\n"); p.stdin.flush()
        res = [p.stdout.readline().split() for p in procs]
    finally:
        for p in procs:
            try:
                p.stdin.close()
            except OSError:
                pass
            p.wait()
    if any(len(r) != 3 or r[0] != "DONE" for r in res):
        raise RuntimeError("cpu baseline child failed")
    n = min(int(r[1]) for r in res)
    dt = max(float(r[2]) / int(r[1]) for r in res)
    return dt / scale, n, sample_cfg, scale, cores


# one HIP kernel per phase name (pop_time_phase); 'vmix' is a multi-kernel phase and is listed only
KERNEL_OF_PHASE = {"tracer_rhs": "k_tracer_rhs_lds", "momentum_rhs": "k_momentum_rhs_lds", "state": "k_state3d",
                   "impvmixu": "k_impvmixu", "add_btrop": "k_add_barotropic"}


def pmc_traffic(workload, kernel):
    """HBM/fabric bytes per launch from the committed rocprofv3 --pmc passes (FETCH_SIZE x2 on gfx950 +
    WRITE_SIZE, separate passes; profiles/r02_pmc_traffic.json).  None when no pass exists for this case."""
    try:
        for name in ("r04_pmc_traffic.json", "r03_pmc_traffic.json", "r02_pmc_traffic.json"):
            path = os.path.join(ROOT, "profiles", name)
            if os.path.exists(path):
                with open(path) as f:
                    t = json.load(f)
                e = t[workload][kernel]
                return e["fetch_bytes"] + e["write_bytes"]
    except (OSError, KeyError, ValueError):
        pass
    return None


def _kill_group(p):
    """end a child we started in its own session, and everything it started (never by pattern: the exact process group)"""
    import signal
    for sig, wait in ((signal.SIGTERM, 5.0), (signal.SIGKILL, 10.0)):
        if p.poll() is not None:
            break
        try:
            os.killpg(p.pid, sig)
        except (ProcessLookupError, PermissionError):
            pass
        try:
            p.wait(timeout=wait)
        except Exception:  # noqa: BLE001
            pass


def _json_line(text):
    for ln in (text or "").splitlines():
        if ln.startswith("{") and '"metric"' in ln:
            return ln
    return None


def self_launch(argv, ngpus):
    """`python bench.py --gpus N` without a launcher (WORLD_SIZE unset): start the N ranks as a CHILD process
    (torchrun, rendezvous on 127.0.0.1) before anything in this process has touched the GPU and relay its JSON line.
    Never an exec: this pool forbids replacing a process image.  Watchdog: the child runs in its own
    process group under a time limit; the ranks inside it already recover from a native-transport failure by themselves
    (`supervise`), so a child that still ends without a line -- rendezvous trouble, a stall the ranks could not see -- is
    killed as a group and ONE fresh child is started with the torch.distributed transport; the line says which child
    produced it.  Exit code non-zero if neither did."""
    import socket
    import subprocess
    t_first = float(os.environ.get("POP_BENCH_LAUNCH_TIMEOUT", "480"))
    t_second = float(os.environ.get("POP_BENCH_RELAUNCH_TIMEOUT", "300"))
    history = []
    for attempt, (limit, extra) in enumerate(((t_first, {}), (t_second, {"POP_BENCH_TRANSPORT": "torch", "POP_BENCH_RELAUNCHED": "1"}))):
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(ngpus),
               "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + argv
        env = dict(os.environ, **extra)
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")      # dmabuf IPC (RCCL across processes on this image)
        env["POP_BENCH_SELF_LAUNCHED"] = "1"
        if history:
            env["POP_BENCH_LAUNCH_HISTORY"] = json.dumps(history)
        p = subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, text=True, start_new_session=True)
        try:
            out, _ = p.communicate(timeout=limit)
            why = "exit code %d" % p.returncode
        except subprocess.TimeoutExpired:
            _kill_group(p)
            out = ""
            try:
                out, _ = p.communicate(timeout=5)
            except Exception:  # noqa: BLE001
                pass
            why = "no line after %d s: process group killed" % int(limit)
        line = _json_line(out)
        if line:
            print(line, flush=True)
            _kill_group(p)
            return 0
        sys.stdout.write(out or "")
        if "POP_BENCH_FATAL" in (out or ""):
            return 3
        history.append({"launch": attempt + 1, "transport": extra.get("POP_BENCH_TRANSPORT", os.environ.get("POP_BENCH_TRANSPORT", "rccl")), "outcome": why})
        print("bench.py: launch %d produced no result line (%s)%s" % (attempt + 1, why, "; starting one fresh child with the torch.distributed transport" if attempt == 0 else ""),
              file=sys.stderr, flush=True)
        if os.environ.get("POP_BENCH_TRANSPORT", "rccl") != "rccl":
            break                                                 # the caller already asked for the fallback transport: nothing else to try
    return 1


def _rdzv_store(world, host_it):
    """the launcher's rendezvous store (torchrun hosts it at MASTER_ADDR:MASTER_PORT and its workers are clients); with a bare
    environment launch nobody hosts one yet, so the rank-0 supervisor does"""
    from datetime import timedelta
    from torch.distributed import TCPStore
    return TCPStore(os.environ.get("MASTER_ADDR", "127.0.0.1"), int(os.environ["MASTER_PORT"]), world_size=None, is_master=host_it,
                    timeout=timedelta(seconds=120), wait_for_workers=False)


def supervise(argv, world):
    """Every rank the launcher started is a SUPERVISOR that never touches the GPU: it runs the real rank as a worker child in its own
    process group under a time limit.  Attempt 1 uses the library's RCCL transport; if rank 0's worker ends without a result line
    (crash, refusal, or a stall: the limit expires) every supervisor kills its worker's process group and all start attempt 2 in
    fresh processes with the torch.distributed transport -- the first real multi-GPU run of the native transport cannot lose the
    measurement (VERDICT r3 #1c, #8).  The supervisors agree through the launcher's store (rank 0 decides: only its worker prints);
    each attempt's workers form their process group under their own key prefix of that store."""
    import subprocess
    rank = int(os.environ.get("RANK", "0"))
    agent_store = os.environ.get("TORCHELASTIC_USE_AGENT_STORE", "") == "True"
    store = _rdzv_store(world, host_it=(rank == 0 and not agent_store))
    first = os.environ.get("POP_BENCH_TRANSPORT", "rccl")
    t1 = float(os.environ.get("POP_BENCH_ATTEMPT_TIMEOUT", "300"))
    t2 = float(os.environ.get("POP_BENCH_FALLBACK_TIMEOUT", "270"))
    attempts = [(first, t1)] + ([("torch", t2)] if first == "rccl" else [])
    history = json.loads(os.environ.get("POP_BENCH_LAUNCH_HISTORY", "[]"))
    for k, (transport, limit) in enumerate(attempts):
        env = dict(os.environ, POP_BENCH_WORKER="1", POP_BENCH_ATTEMPT=str(k), POP_BENCH_TRANSPORT=transport,
                   POP_BENCH_HISTORY=json.dumps(history))
        p = subprocess.Popen([sys.executable, os.path.abspath(__file__)] + argv, env=env, start_new_session=True,
                             stdout=subprocess.PIPE if rank == 0 else None, text=True)
        key = "pop_bench/verdict/%d" % k
        t0 = time.time()
        if rank == 0:
            try:
                out, _ = p.communicate(timeout=limit)
                why = "worker exit code %d" % p.returncode
            except subprocess.TimeoutExpired:
                _kill_group(p)
                out = ""
                try:
                    out, _ = p.communicate(timeout=5)
                except Exception:  # noqa: BLE001
                    pass
                why = "no result line within %d s (stalled): worker process groups killed" % int(limit)
            line = _json_line(out)
            fatal = not line and p.returncode == 3
            store.set(key, "ok" if line else "fatal" if fatal else "fail:" + why)
            if line:
                print(line, flush=True)
                _kill_group(p)
                return 0
            if fatal:
                print("POP_BENCH_FATAL", flush=True)              # read by self_launch: do not launch again
                return 3
            sys.stdout.write(out or "")
            print("bench.py rank 0: attempt %d (%s transport) gave no result line: %s" % (k + 1, transport, why), file=sys.stderr, flush=True)
            history.append({"attempt": k + 1, "transport": transport, "outcome": why})
        else:
            verdict = None
            while verdict is None and time.time() - t0 < limit + 60.0:
                if store.check([key]):
                    verdict = store.get(key).decode()
                else:
                    time.sleep(0.5)
            if verdict == "ok":
                try:
                    p.wait(timeout=20)                             # the result is out; a worker still busy tearing down is not waited for
                except subprocess.TimeoutExpired:
                    pass
                _kill_group(p)
                return 0
            _kill_group(p)
            history.append({"attempt": k + 1, "transport": transport, "outcome": verdict or "no verdict from rank 0"})
            if verdict is None:
                return 1
            if verdict == "fatal":
                return 3
        time.sleep(2.0)                                           # the killed workers' device memory is released with their processes
    return 1


def tensor_view(torch, ptr, shape):
    """torch tensor over a device pointer of the library (pop_field_device_ptr), float64, C order"""
    class _Holder:
        pass
    h = _Holder()
    h.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": "<f8", "data": (int(ptr), False), "version": 2, "strides": None}
    return torch.as_tensor(h, device="cuda")


def kpp_deep_state(pkg, model, cfg, torch, nlev=12, warm=6, steps=8):
    """Second, separately labelled measurement AFTER the timed region: the same workload on a state whose KPP boundary layer is
    several levels deep (surface cooling over a weakly stratified upper ocean in latitude bands; profiles/kpp_deep.py), because
    the headline state (STF = 0) keeps HBLT at its minimum, the best case for the on-demand forms of the KPP kernels.
    The tracers are edited in place on the GPU through pop_field_device_ptr."""
    nb, km, ny, nx = model.nblocks, model.km, model.nyb, model.nxb
    kmt_h = model.geti("KMT")
    kmt = torch.as_tensor(kmt_h, device="cuda")
    tlat_h = np.broadcast_to(np.linspace(-1.35, 1.5, ny)[None, :, None], (nb, ny, nx)).copy()
    band = torch.as_tensor(np.sin(3.0 * tlat_h) > 0.0, device="cuda")
    z = torch.arange(nlev, device="cuda", dtype=torch.float64)[None, :, None, None]
    cond = (z < kmt[:, None].to(torch.float64)) & band[:, None]
    model.sync()
    for tl in (0, 1, 2):
        for n, slope in ((0, 2.0e-4), (1, -2.0e-9)):
            ptr = model.L.pop_field_device_ptr(model.h, b"TRACER", tl, n)
            T = tensor_view(torch, ptr, (nb, km, ny, nx))
            top = T[:, :nlev]
            top.copy_(torch.where(cond, T[:, 0:1] - slope * z, top))
    torch.cuda.synchronize()
    del kmt, band, cond
    model.set("STF", -3.0e-2 * np.sin(tlat_h) - 1.0e-2, n=0)
    model.set("STF", 2.0e-6 * np.cos(2.0 * tlat_h), n=1)
    for _ in range(warm):
        model.step()
    model.sync()
    model.scalar("solver_ms_reset")
    t0 = time.perf_counter()
    its = []
    for _ in range(steps):
        model.step()
        its.append(model.solver_diagnostics()[0])
    model.sync()
    ms = 1e3 * (time.perf_counter() - t0) / steps
    oc = kmt_h > 0
    kbl = model.geti("KBL")[oc]
    H = model.get("HBLT")[oc]
    sol_ms = model.scalar("solver_ms_total") / max(model.scalar("solver_calls_total"), 1.0)
    return {"what": "same workload, KPP boundary layer several levels deep (surface cooling over a weakly stratified upper %d levels in "
                    "latitude bands, profiles/kpp_deep.py); measured AFTER the timed region, not the headline" % nlev,
            "ms_per_step": round(ms, 3), "steps": steps, "warmup": warm, "pcg_iters_per_step": float(np.mean(its)),
            "solver_ms_per_step": round(sol_ms, 3), "ms_per_step_without_solver": round(ms - sol_ms, 3),
            "hblt_level_p50": int(np.percentile(kbl, 50)), "hblt_level_p90": int(np.percentile(kbl, 90)), "hblt_level_max": int(kbl.max()),
            "hblt_m_p50": round(float(np.median(H)) / 100, 1), "hblt_m_p90": round(float(np.percentile(H, 90)) / 100, 1)}


DUMP_BYTES = 56 << 20     # --dump-outputs: all arrays together, under the 64 MB a dump may hold


def dump_names(cfg):
    return [("TEMP", "SALT")[n] if n < 2 else "TRACER_%d" % n for n in range(cfg.nt)] + ["UVEL", "VVEL", "PSURF", "UBTROP", "VBTROP"]


def dump_cells(model, cfg, per_array, seed=0):
    """The cells --dump-outputs writes, as flat offsets into this rank's local field arrays: "t3" / "u3" the 3-D ocean cells of the
    T / U grid (k < KMT / KMU), "t2" / "u2" the ocean columns.  Global (j, i, k) order; where a grid has more than per_array of them,
    a sample of per_array drawn with a fixed seed -- the same cells in every run with the same arguments, whatever the blocks."""
    km, n2, nx = model.km, model.nyb * model.nxb, model.nxb
    where = np.full((cfg.ny_global, cfg.nx_global), -1, dtype=np.int64)   # global (j, i) -> offset in a local 2-D array; -1: not held here
    for bid in model.local_block_ids():
        B = model.get_block(bid)
        jj, ii = np.arange(B["jb"] - 1, B["je"]), np.arange(B["ib"] - 1, B["ie"])
        where[np.ix_(B["j_glob"][jj] - 1, B["i_glob"][ii] - 1)] = (B["local_id"] - 1) * n2 + jj[:, None] * nx + ii[None, :]
    where = where.ravel()
    held = where >= 0
    rng = np.random.default_rng(seed)

    def cells(levels, nz):              # levels (nblocks, ny_block, nx_block): ocean cells per column; nz: levels of the array
        depth = np.zeros(where.size, dtype=np.int64)
        depth[held] = levels.ravel()[where[held]]
        end = np.cumsum(depth)
        total = int(end[-1])
        r = np.arange(total) if total <= per_array else np.sort(rng.choice(total, per_array, replace=False))
        col = np.searchsorted(end, r, side="right")
        k = r - (end[col] - depth[col])
        return where[col] // n2 * (nz * n2) + k * n2 + where[col] % n2

    kmt, kmu = model.geti("KMT"), model.geti("KMU")
    return {"t3": cells(kmt, km), "u3": cells(kmu, km), "t2": cells(kmt > 0, 1), "u2": cells(kmu > 0, 1)}


def dump_outputs(model, cfg, out_dir):
    """--dump-outputs: the prognostic state the last timed step left -- logical time level 'cur', what the next step starts from --
    as out_dir/<name>.npy (float64) over the cells of dump_cells.  Read with pop_get_field, which changes nothing that --full measures."""
    names = dump_names(cfg)
    sel = dump_cells(model, cfg, DUMP_BYTES // 8 // len(names))
    n3 = model.nblocks * model.km * model.nyb * model.nxb
    buf = np.empty(n3)
    fields = [("TRACER", n, "t3", n3) for n in range(cfg.nt)] + [("UVEL", 0, "u3", n3), ("VVEL", 0, "u3", n3), ("PSURF", 0, "t2", n3 // model.km),
                                                                  ("UBTROP", 0, "u2", n3 // model.km), ("VBTROP", 0, "u2", n3 // model.km)]
    os.makedirs(out_dir, exist_ok=True)
    for name, (field, n, grid, count) in zip(names, fields):
        model._chk(model.L.pop_get_field(model.h, field.encode(), 1, n, buf.ctypes.data_as(C.POINTER(C.c_double)), count))
        np.save(os.path.join(out_dir, name + ".npy"), buf[:count][sel[grid]])


def roofline(pkg, model, cfg, workload, world, elapsed, steps, land_frac):
    """--full: every 3-D phase kernel timed with HIP events on its launch stream (pop_time_phase: the kernel launches only, in runs of
    their own after the timed steps) against SURVEY.md 8(d)'s algorithmic bytes, and the barotropic solver of the timed steps"""
    solver_ms = model.scalar("solver_ms_total")
    solver_iters = model.scalar("solver_iterations_total")
    solver_calls = model.scalar("solver_calls_total")
    ms_step = 1e3 * elapsed / steps
    vm = cfg.vmix_choice - 1
    ncell_phys = cfg.nx_global * cfg.ny_global * cfg.km // world
    ncell_phys = int(round(ncell_phys * (1.0 - land_frac)))
    phases = {}
    extra_words = {}
    for ph, words in PHASE_WORDS.items():
        if ph == "impvmixt" and not cfg.lpressure_avg:
            continue
        try:
            ms = model.time_phase(ph, reps=10)
        except pkg.PopError:
            continue
        nw = words[vm]        # SURVEY.md 8(d) words of the phase -- the only count `frac` uses
        gb = nw * 8.0 * ncell_phys / 1e9
        phases[ph] = {"ms": round(ms, 4), "alg_GB": round(gb, 4), "GBps": round(gb / (ms * 1e-3), 1), "alg_words": nw}
        # del4 on large grids: the tracer / momentum launch also READS the two first-Laplacian fields and WRITES the next step's
        # (the output of k_del4_d2t / k_del4_d2u, which are then not launched).  SURVEY 8(d) has no del4 row, so these words are
        # reported beside the phase, never inside `frac`.
        if ph == "tracer_rhs" and cfg.hmix_tracer == 4:
            extra_words[ph] = 2 + (2 if model.dim("d2t_last_formed") else 0)
        if ph == "momentum_rhs" and cfg.hmix_momentum == 4:
            extra_words[ph] = 2 + (2 if model.dim("d2u_last_formed") else 0)
        if ph in extra_words:
            phases[ph]["del4_extra_words_moved"] = extra_words[ph]
    # dominant single baroclinic stencil kernel (north_star: "fraction of HBM roofline for the baroclinic stencil")
    dom = max((k for k in phases if k in ("tracer_rhs", "momentum_rhs")), key=lambda k: phases[k]["ms"])
    kern = KERNEL_OF_PHASE[dom]
    roof = {"bound": "hbm", "kernel": kern, "achieved": phases[dom]["GBps"], "peak": HBM_PEAK_GBS, "unit": "GB/s",
            "frac": round(phases[dom]["GBps"] / HBM_PEAK_GBS, 4),
            "frac_definition": "SURVEY.md 8(d) words of the phase (E = 10, B = 12) x 8 B x computed cells / HIP-event launch time / 8 TB/s",
            "traffic": pmc_traffic(workload, kern) if world == 1 else None,
            "traffic_source": "rocprofv3 --pmc FETCH_SIZE(x2)/WRITE_SIZE passes of `bench.py --profile-run headline` (separate runs, profiles/collect_r04.sh): committed profiles/r04_pmc_traffic.json (r03 if absent), not measured in this process",
            "alg_bytes_per_launch": phases[dom]["alg_GB"] * 1e9, "avg_launch_ms": phases[dom]["ms"], "phases": phases}
    if dom in extra_words:
        w = phases[dom]["alg_words"] + extra_words[dom]
        roof["frac_all_words_moved"] = round(w * 8.0 * ncell_phys / 1e9 / (phases[dom]["ms"] * 1e-3) / HBM_PEAK_GBS, 4)
        roof["all_words_moved"] = w
    # both baroclinic stencil kernels together (tracer + momentum right-hand sides): 8(d) bytes / summed time
    pair_gb = phases["tracer_rhs"]["alg_GB"] + phases["momentum_rhs"]["alg_GB"]
    pair_ms = phases["tracer_rhs"]["ms"] + phases["momentum_rhs"]["ms"]
    roof["baroclinic_stencils"] = {"kernels": [KERNEL_OF_PHASE["tracer_rhs"], KERNEL_OF_PHASE["momentum_rhs"]],
                                   "achieved": round(pair_gb / (pair_ms * 1e-3), 1), "frac": round(pair_gb / (pair_ms * 1e-3) / HBM_PEAK_GBS, 4)}
    step_words = sum(v[vm] for k, v in PHASE_WORDS.items() if k in phases)
    roof["step_alg_GBps"] = round(step_words * 8.0 * ncell_phys * world / 1e9 / (elapsed / steps), 1)
    # the barotropic solver ("iterations x per-iteration time separately"; 14 words = 112 B per 2-D point per iteration)
    if solver_calls > 0 and solver_iters > 0:
        pts = int(round(cfg.nx_global * cfg.ny_global // world * (1.0 - land_frac)))
        us_it = 1e3 * solver_ms / solver_iters
        sol = {"solver": ["pcg", "ChronGear", "PCSI"][cfg.solver_choice - 1], "iterations_per_step": round(solver_iters / solver_calls, 2),
               "ms_per_step": round(solver_ms / solver_calls, 4), "us_per_iteration": round(us_it, 2),
               "timing": "HIP events around POP_SolversRun on the launch stream inside the timed steps (start-up, checks and the final halo included)",
               "alg_bytes_per_iteration": 112 * pts, "active_points": pts,
               "achieved": round(112 * pts / 1e9 / (us_it * 1e-6), 1), "unit": "GB/s",
               "frac": round(112 * pts / 1e9 / (us_it * 1e-6) / HBM_PEAK_GBS, 4), "share_of_step": round(solver_ms / solver_calls / ms_step, 4)}
        try:
            sol["k_block_sums_us_isolated"] = round(1e3 * model.time_phase("block_sums", reps=50), 2)
            sol["k_block_sums_launches_per_iteration"] = 2 if cfg.solver_choice == 1 else (1 if cfg.solver_choice == 2 else 0)
        except pkg.PopError:
            pass
        roof["solver"] = sol
    return roof


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)   # land elimination starts with the fifth step (four steps write the land values)
    ap.add_argument("--workload", default=os.environ.get("POP_BENCH_WORKLOAD", "tx0.1v3"))
    ap.add_argument("--solver", default=os.environ.get("POP_BENCH_SOLVER", "pcg"), choices=["pcg", "chrongear", "pcsi"],
                    help="barotropic solver (headline = pcg, BASELINE.json north_star)")
    ap.add_argument("--precond", default=os.environ.get("POP_BENCH_PRECOND", "diagonal"), choices=["diagonal", "evp"],
                    help="solver preconditioner (headline = diagonal)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--block-rows", type=int, default=0, help="rows per j-band block (default: one band per rank, or balanced bands on large grids)")
    ap.add_argument("--no-deep-state", action="store_true", help="skip the second (deep KPP boundary layer) measurement after the timed region")
    ap.add_argument("--profile-run", default="", choices=["", "headline", "deep"],
                    help="under rocprofv3 only (profiles/collect_r04.sh): nothing but step launches of ONE state in the process -- no per-phase "
                         "HIP-event repetitions, no CPU baseline; 'deep' edits the state to the deep-boundary-layer one before the steps.  The line "
                         "then carries no roofline object and is not a bench line")
    ap.add_argument("--gm", nargs="?", const="constant", default="", choices=["constant", "cesm"], help="NOT the headline: Gent-McWilliams + isopycnal tracer mixing (hmix_tracer = 3, SURVEY 8 f4) in place of del2 / del4; "
                                                      "config.hmix_tracer says so in the line")
    ap.add_argument("--pbc", action="store_true", help="NOT the headline: partial bottom cells on stepped bathymetry (grid_nml partial_bottom_cells, SURVEY 8 f3); "
                                                       "config.partial_bottom_cells says so in the line")
    ap.add_argument("--tmix", default="", choices=["", "avg", "avgfit", "robert"], help="NOT the headline: time_mix_opt (default: the workload's, avgfit); 'robert' = the Robert-Asselin-Williams "
                                                                                      "filter step (SURVEY 8 f2), CESM's default on gx1v7; config.time_mix says so")
    ap.add_argument("--tadvect", default="", choices=["", "centered", "upwind3", "lw_lim"], help="NOT the headline: tracer advection (default centred); 'upwind3' is CESM's default on the gx grids")
    ap.add_argument("--grid-input", action="store_true", help="NOT the headline: horizontal grid and bathymetry supplied by the caller (pop_create_with_grid; the synthetic "
                                                              "lat-lon arrays of tests/popcfg.synthetic_grid) instead of the internal grid; config.grid_input says so")
    ap.add_argument("--tripole", action="store_true", help="NOT the headline: tripole northern boundary (ns_boundary_type 'tripole') on the --grid-input arrays")
    ap.add_argument("--full", action="store_true", help="also measure what the headline does not need, after the timed steps: the roofline (per-phase "
                                                        "kernel times), the deep KPP boundary-layer state and the CPU baseline")
    ap.add_argument("--dump-outputs", metavar="DIR", default="", help="write the state the last timed step left as DIR/<name>.npy (float64, ocean "
                                                                     "cells; a fixed seeded sample of them on large grids); one GPU only")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")
    if args.dump_outputs and (args.gpus != 1 or args.profile_run):
        ap.error("--dump-outputs needs --gpus 1 and no --profile-run")

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ and "RANK" not in os.environ:
        # no launcher around us: become one (child process; nothing here has touched the GPU yet, torch is not even imported)
        raise SystemExit(self_launch(sys.argv[1:], args.gpus))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit("--gpus %d but WORLD_SIZE=%d (launch with torch.distributed.run, or with no launcher at all)" % (args.gpus, world))
    worker = os.environ.get("POP_BENCH_WORKER") == "1"
    if world > 1 and not worker and os.environ.get("POP_BENCH_NO_SUPERVISOR") != "1":
        # a rank as the launcher started it: supervise the real rank (a worker child) -- see supervise(); this process never touches the GPU
        raise SystemExit(supervise(sys.argv[1:], world))

    import faulthandler
    import torch
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world > 1:
        # where a stalled rank was: python stacks of every thread on stderr before the supervisor's limit expires (diagnosis only)
        faulthandler.dump_traceback_later(float(os.environ.get("POP_BENCH_STALL_DUMP", "240")), exit=False)
    hang = os.environ.get("POP_BENCH_TEST_HANG", "")              # tests only: "<attempt>:<rank>" stalls there, as a wedged transport would
    if not torch.cuda.is_available():
        print("bench.py needs a GPU: libpop_amd has no CPU fallback", file=sys.stderr)
        raise SystemExit(3)                                        # 3 = cannot run here at all: no other transport or launch will help
    # POP_BENCH_BACKEND=gloo: CPU-staged transport so the N>1 path can be rehearsed on a 1-GPU box
    backend = os.environ.get("POP_BENCH_BACKEND", "nccl")
    dev = local % torch.cuda.device_count()
    torch.cuda.set_device(dev)
    dist = None
    if world > 1:
        import torch.distributed as dist
        kw = {}
        if worker:   # this attempt's process group under its own key prefix of the launcher's store (a second attempt must not read the first one's keys)
            kw = dict(store=dist.PrefixStore("pop_bench/attempt%s" % os.environ.get("POP_BENCH_ATTEMPT", "0"), _rdzv_store(world, False)),
                      rank=rank, world_size=world)
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", dev), **kw)
        else:
            dist.init_process_group("gloo", **kw)
        if hang and hang == "%s:%d" % (os.environ.get("POP_BENCH_ATTEMPT", "0"), rank):
            time.sleep(10 ** 6)

    import __graft_entry__ as ge
    pkg = ge.load_package()
    cfg = workload_config(args.workload, world, args.block_rows)
    cfg.solver_choice = {"pcg": 1, "chrongear": 2, "pcsi": 3}[args.solver]
    cfg.preconditioner_choice = 1 if args.precond == "evp" else 0
    if args.pbc and args.gm:
        raise SystemExit("--gm with --pbc: the reference refuses Gent-McWilliams with partial bottom cells (hmix_gm.F90:782-785), so does the library")
    if args.pbc:
        cfg.partial_bottom_cells = 1
    if args.gm:   # the 1-degree production tracer mixing (namelist_defaults_pop.xml hmix_tracer_choice 'gm' on the gx grids)
        cfg.hmix_tracer, cfg.ah = 3, 0.8e7
        if args.gm == "cesm":   # the namelist defaults of the gx grids: transition layer + buoyancy-frequency-dependent kappa recomputed once a day
            cfg.gm_transition_layer, cfg.gm_kappa_type, cfg.gm_kappa_freq = 1, 1, 2
    if args.tmix:
        cfg.tmix_opt = {"avg": 1, "avgfit": 2, "robert": 3}[args.tmix]
    if args.tadvect:
        cfg.tadvect = {"centered": 1, "upwind3": 2, "lw_lim": 3}[args.tadvect]
    grid = None
    if args.tripole or args.grid_input:
        from popcfg import synthetic_grid
        if args.tripole:
            cfg.ns_boundary = 2
        grid = synthetic_grid(cfg)
    model = pkg.PopModel(cfg, rank=rank, nranks=world, grid=grid)
    del grid
    comm, transport, transport_note = None, "none", ""
    if world > 1:
        # default: the library's own RCCL transport (stream-ordered ncclSend/Recv/AllReduce, no host call per
        # message); POP_BENCH_TRANSPORT=torch keeps the torch.distributed callbacks.  A failed self-test on
        # any rank makes every rank fall back to the callbacks.
        # (POP_BENCH_BACKEND=gloo + POP_RCCL_LIB=tests/rccl_stub/librccl_stub.so rehearses this branch with several
        # ranks on a one-GPU box: torch's own process group is then gloo, the library binds the stand-in.)
        want_native = (backend == "nccl" or os.environ.get("POP_RCCL_LIB")) and os.environ.get("POP_BENCH_TRANSPORT", "rccl") == "rccl"
        ok = 0
        if want_native:
            box = [None]
            if rank == 0:
                try:
                    box[0] = pkg.PopModel.rccl_unique_id()
                except pkg.PopError as e:
                    transport_note = "rccl transport unavailable: %s" % e
                    print(transport_note, file=sys.stderr)
            dist.broadcast_object_list(box, src=0)
            if box[0] is not None:
                try:
                    model.comm_init_rccl(box[0])
                    model.comm_selftest()
                    ok = 1
                except pkg.PopError as e:
                    transport_note = "rank %d: rccl transport failed its self-test: %s" % (rank, e)
                    print(transport_note, file=sys.stderr)
            t = torch.tensor([ok], dtype=torch.int32, device="cuda" if backend == "nccl" else "cpu")
            dist.all_reduce(t, op=dist.ReduceOp.MIN)
            ok = int(t.item())
        if ok:
            transport = "rccl-native"
        else:
            comm = TorchComm(pkg, model, rank, world, staged=(backend != "nccl"))  # noqa: F841
            transport = "torch.distributed/" + backend
            if not want_native:
                transport_note = "native transport not requested (POP_BENCH_TRANSPORT / POP_BENCH_BACKEND)"
            notes = [None] * world
            dist.all_gather_object(notes, transport_note)
            transport_note = "; ".join(n for n in notes if n) or "native self-test failed on another rank"

    def barrier():
        model.sync()
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
            torch.cuda.synchronize()

    if args.profile_run:
        if args.profile_run == "deep":
            kpp_deep_state(pkg, model, cfg, torch, warm=max(args.warmup, 6), steps=args.steps)
        else:
            for _ in range(args.warmup + args.steps):
                model.step()
        model.sync()
        print(json.dumps({"profile_run": args.profile_run, "workload": args.workload, "steps": args.steps, "warmup": args.warmup}))
        model.close()
        return
    iters = []
    for _ in range(args.warmup):
        model.step()
    barrier()
    model.scalar("solver_ms_reset")
    t0 = time.perf_counter()
    for _ in range(args.steps):
        model.step()
        iters.append(model.solver_diagnostics()[0])
    model.sync()
    busy = time.perf_counter() - t0          # this rank's own work done (before it waits for the others)
    barrier()
    elapsed = time.perf_counter() - t0
    rank_ms = [1e3 * busy / args.steps]
    if dist is not None:
        t = torch.tensor([elapsed], dtype=torch.float64, device="cuda" if backend == "nccl" else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
        rank_ms = [None] * world
        dist.all_gather_object(rank_ms, 1e3 * busy / args.steps)
    if args.dump_outputs:
        dump_outputs(model, cfg, args.dump_outputs)
    # per-rank evidence for the record: ocean columns owned, what the transport reports about itself
    kmt_phys = model.geti("KMT")[:, 2:-2, 2:-2]
    ocean_cols = [int((kmt_phys > 0).sum())]
    cinfo = [model.comm_info()]
    # which code path every rank really ran (the shape limits fall back silently otherwise)
    mine = {"blocks": model.local_block_ids(), "solver_path": {0: "none", 1: "operation by operation", 2: "fused (single rank)", 3: "fused, blocks spread over ranks",
                                                              4: "replicated fused solve on every rank"}.get(model.dim("solver_path"), "?"),
            "thomas_tracers": "register" if model.dim("thomas_register_tracers") == 1 else "generic (HBM scratch)",
            "thomas_velocity": "register" if model.dim("thomas_register_velocity") == 1 else "generic (HBM scratch)",
            "pcg_resident_launch": bool(model.dim("pcg_persist_used") == 1),      # small 2-D systems: the whole solve as one resident launch (kernels_pcg_persist.hpp)
            "device": dev}
    paths = [mine]
    if dist is not None:
        ocean_cols, cinfo, paths = [None] * world, [None] * world, [None] * world
        dist.all_gather_object(ocean_cols, int((kmt_phys > 0).sum()))
        dist.all_gather_object(cinfo, model.comm_info())
        dist.all_gather_object(paths, mine)
    ms_step = 1e3 * elapsed / args.steps
    # step calls per model day: with time_mix_opt = 'avgfit' a day is `full` leapfrog steps plus `half` averaging
    # half-steps (time_management.F90:820-860; tx0.1v3: 300 + 19 = 319 calls), every one a full pass of the hot path
    calls_per_day = model.dim("nsteps_per_interval")
    sypd = 86400.0 / ((elapsed / args.steps) * calls_per_day * 365.0)

    vm = cfg.vmix_choice - 1
    ncell_local = model.nxb * model.nyb * model.km * model.nblocks
    # land elimination: once it is active (after the first steps) workgroups whose 64-column row segment holds no ocean cell
    # do not run, so the algorithmic bytes are counted over the segments that do -- the units the launches process
    land_frac = model.scalar("land_tile_fraction") if model.dim("land_skip_active") else 0.0
    # headline state: where the KPP boundary layer sits (decides how much the on-demand KPP forms save)
    hblt_levels = None
    if vm == 2:
        kbl = model.geti("KBL")[model.geti("KMT") > 0]
        if kbl.size:
            hblt_levels = [int(np.percentile(kbl, q)) for q in (50, 90, 100)]
    roof = roofline(pkg, model, cfg, args.workload, world, elapsed, args.steps, land_frac) if args.full else None

    tun = {k: v for k, v in model.tuning().items() if v is not None and k != "struct_bytes"}
    out = {
        "metric": "simulated_years_per_day", "value": round(sypd, 3), "unit": "SYPD",
        "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(ms_step, 4),
        "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": "f64", "data": "synthetic",
        "config": {"workload": args.workload, "grid": [cfg.nx_global, cfg.ny_global, cfg.km], "nt": cfg.nt,
                   "block_size": [cfg.block_size_x, cfg.block_size_y], "steps_per_day": cfg.steps_per_day, "step_calls_per_day": calls_per_day,
                   "land_tile_fraction": round(land_frac, 4), "distribution": "balanced-ocean-columns" if cfg.distribution_type else "equal-block-counts",
                   "blocks_local": model.nblocks,
                   "hmix": "del%d" % cfg.hmix_momentum, "hmix_tracer": {2: "del2", 3: "gm" + ("(transition layer, bfre kappa once a day)" if cfg.gm_transition_layer else "(constant kappa)"), 4: "del4"}[cfg.hmix_tracer], "vmix": ["const", "rich", "kpp"][vm],
                   "partial_bottom_cells": bool(cfg.partial_bottom_cells), "ns_boundary": ["closed", "cyclic", "tripole"][cfg.ns_boundary],
                   "grid_input": bool(args.tripole or args.grid_input), "time_mix": ["", "avg", "avgfit", "robert"][cfg.tmix_opt], "tadvect": ["", "centered", "upwind3", "lw_lim"][cfg.tadvect], "pcsi_two_iterations_per_launch": bool(model.dim("pcsi_two_step")) if cfg.solver_choice == 3 else None, "solver": ["pcg", "ChronGear", "PCSI"][cfg.solver_choice - 1], "preconditioner": args.precond, "pcg_iters_per_step": float(np.mean(iters)),
                   "cells_local_with_ghosts": ncell_local, "transport": transport,
                   # every output of the step is bitwise what the full evaluation gives (tests/test_gpu_parity.py); DESIGN.md 3, "KPP's surface-layer buoyancy difference on demand"
                   "kpp_surface_buoyancy": ("on-demand down to the boundary-layer depth" if vm == 2 and tun.get("kpp_lazy", 1) != 0
                                            and not cfg.lcheckekmo and cfg.kpp_ml_diagnostics != 1 else "every level"),
                   "tuning_overrides": tun},
    }
    if roof is not None:
        out["roofline"] = roof
    out["config"]["code_paths"] = {k: v for k, v in mine.items() if k != "blocks"}
    if hblt_levels is not None:
        out["config"]["hblt_level_p50"], out["config"]["hblt_level_p90"], out["config"]["hblt_level_max"] = hblt_levels
        out["config"]["hblt_note"] = "STF = 0 (SURVEY 8d) keeps the KPP boundary layer at its minimum: the best case for the on-demand KPP forms; see kpp_deep_state"
    if world > 1:
        out["multi_gpu"] = {"transport": transport, "transport_note": transport_note, "launcher": "self (child torch.distributed.run)" if os.environ.get("POP_BENCH_SELF_LAUNCHED") else "external",
                            "ranks": world, "ncclCommCount": [ci["ncclCommCount"] for ci in cinfo],
                            "ncclCommCount_second_communicator": [ci["ncclCommCount_second_communicator"] for ci in cinfo],
                            "librccl": cinfo[0]["librccl"], "halo_neighbour_ranks": [ci["halo_neighbour_ranks"] for ci in cinfo],
                            "midstep_halo_overlap": [ci["midstep_halo_overlap"] for ci in cinfo],
                            "ocean_columns_per_rank": ocean_cols, "rank_ms_per_step": [round(x, 3) for x in rank_ms],
                            "per_rank": paths, "max_blocks_per_rank": model.dim("max_blocks_per_rank"),
                            "attempt": int(os.environ.get("POP_BENCH_ATTEMPT", "0")) + 1,
                            "earlier_attempts": json.loads(os.environ.get("POP_BENCH_HISTORY", "[]")),
                            "supervised": worker,
                            "rank_ms_max_over_min": round(max(rank_ms) / max(min(rank_ms), 1e-9), 3),
                            "devices_visible": torch.cuda.device_count()}
    if args.full and world == 1 and rank == 0 and vm == 2 and not args.no_deep_state and args.workload == "tx0.1v3":
        try:
            out["kpp_deep_state"] = kpp_deep_state(pkg, model, cfg, torch)
        except Exception as e:  # noqa: BLE001  (a second measurement must never lose the headline line)
            out["kpp_deep_state"] = {"error": "%s: %s" % (type(e).__name__, e)}
    if args.full and world == 1 and rank == 0 and not args.no_cpu_baseline:
        try:
            dt, n, scfg, scale, cores = cpu_baseline(cfg)
            build = "-O3 -march=x86-64-v3"
        except RuntimeError:                      # e.g. a host without AVX2: the portable -O2 build
            dt, n, scfg, scale, cores = cpu_baseline(cfg, use_o3=False)
            build = "-O2"
        what = "%d concurrent %dx%dx%d sub-domains of %s, one per core (same options; together %.4f of the columns, " \
               "step time scaled by that ratio)" % (cores, scfg.nx_global, scfg.ny_global, scfg.km, args.workload, scale)
        out["cpu_baseline"] = {"value": round(86400.0 / (dt * calls_per_day * 365.0), 5), "unit": "SYPD",
                               "ms_per_step": round(dt * 1e3, 2), "cores": cores, "kind": "port",
                               "sample": "%d leapfrog steps of %s; C oracle at %s (restated reference algorithm, "
                                         "not the upstream binary), one process per core = the block decomposition of an MPI run "
                                         "without its messages" % (n, what, build)}
    if rank == 0:
        print(json.dumps(out))
    model.close()
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
