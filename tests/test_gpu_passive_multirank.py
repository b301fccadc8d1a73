"""Passive tracers and ideal age over several ranks (tests/mr_gpu_passive.py): nt = 4, tracer 3 ideal age, tracer 4 a plain passive
tracer with a field; every tracer of every rank's blocks is bit for bit that of the single-rank run."""
import os

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("nranks,kw", [
    (2, "nt=4"),
    (4, "nt=4,block_size_x=24,block_size_y=20"),
    (2, "nt=4,vmix_choice=3,km=24"),
    (4, "nt=4,vmix_choice=3,km=24,block_size_x=24,block_size_y=20"),
], ids=["2-default", "4-default", "2-kpp", "4-kpp"])
def test_ranks_equal_single_rank(nranks, kw):
    from test_gpu_multirank import _run_check
    out = _run_check(["--nproc-per-node", str(nranks), os.path.join(ROOT, "tests", "mr_gpu_passive.py"),
                "--config", "tiny", "--steps", "3", "--no-restart", "--kw", kw], 300)
    assert "no passive tracer was compared" not in out, out[-2000:]
