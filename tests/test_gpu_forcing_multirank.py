"""Coupled surface forcing over several ranks (tests/mr_gpu_forcing.py): every imported and combined field, the marginal-sea transports and cell values (case salt), and the per-step phase with
ice formation on, are bit for bit those of the single-rank run on every cell of the rank's blocks, ghost cells included."""
import os

import pytest

from mr_launch import ROOT, run_check

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", ["fw-ice", "salt"])
def test_two_ranks_equal_single_rank(case):
    run_check(["--nproc-per-node", "2", os.path.join(ROOT, "tests", "mr_gpu_forcing.py"), "--case", case], 300)
