"""Frazil ice formation over several ranks (tests/mr_gpu_ice.py): ice forms inside the step on every rank, and T, S, RHO, QICE and AQICE
of every rank's blocks are bit for bit those of the single-rank run, ghost rows included.  Without the Robert filter QICE and AQICE
travel in the step tail's bundled halo update; with it ice forms on whole blocks after the updates; the tripole grid mirrors the ghost
rows of the northern blocks."""
import os

import pytest

from mr_launch import ROOT, run_check

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("nranks,kw,grid", [
    (2, "", 0),
    (4, "block_size_x=24,block_size_y=20", 0),
    (2, "tmix_opt=3", 0),
    (4, "tmix_opt=3,block_size_x=24,block_size_y=20", 0),
    (2, "ns_boundary=2", 1),                        # the caller-supplied grid, no wind (tests/mr_gpu_check.py)
    (4, "ns_boundary=2", 1),                        # 4 x 4 blocks, a row of blocks per rank: the fold has one owner
], ids=["2-default", "4-default", "2-robert", "4-robert", "2-tripole", "4-tripole"])
def test_ranks_equal_single_rank(nranks, kw, grid):
    out = run_check(["--nproc-per-node", str(nranks), os.path.join(ROOT, "tests", "mr_gpu_ice.py"),
                     "--config", "tiny", "--steps", "3", "--no-restart", "--grid", str(grid), "--kw", kw], 300)
    assert "no ice field was compared" not in out, out[-2000:]
