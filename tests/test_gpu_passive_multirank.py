"""Passive tracers and ideal age over several ranks (tests/mr_gpu_passive.py): tracer 3 ideal age, every further passive tracer a plain
one with a field (tracer 4 F, tracer 5 2 F); every tracer of every rank's blocks is bit for bit that of the single-rank run.  Beside the
default scheme and KPP: del4 (the first Laplacian of a passive pair needs its own exchange), Gent-McWilliams with KPP, lw_lim with the
Robert filter (one global sum per tracer), an odd tracer count (the launch of one), and nt = 4 through the tripole fold."""
import os

import pytest

from mr_launch import ROOT, run_check

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("nranks,kw,grid", [
    (2, "nt=4", 0),
    (4, "nt=4,block_size_x=24,block_size_y=20", 0),
    (2, "nt=4,vmix_choice=3,km=24", 0),
    (4, "nt=4,vmix_choice=3,km=24,block_size_x=24,block_size_y=20", 0),
    (2, "nt=5,hmix_tracer=4,ah=-1.0e21", 0),
    (2, "nt=5,hmix_tracer=3,vmix_choice=3,km=24", 0),
    (2, "nt=5,tadvect=3,tmix_opt=3", 0),
    (2, "nt=4,ns_boundary=2", 1),                   # as the tripole row of tests/test_gpu_aniso.py: the caller-supplied grid, no wind
], ids=["2-default", "4-default", "2-kpp", "4-kpp", "2-nt5-del4", "2-nt5-gm-kpp", "2-nt5-lw_lim-robert", "2-nt4-tripole"])
def test_ranks_equal_single_rank(nranks, kw, grid):
    out = run_check(["--nproc-per-node", str(nranks), os.path.join(ROOT, "tests", "mr_gpu_passive.py"),
                "--config", "tiny", "--steps", "3", "--no-restart", "--grid", str(grid), "--kw", kw], 300)
    assert "no passive tracer was compared" not in out, out[-2000:]
