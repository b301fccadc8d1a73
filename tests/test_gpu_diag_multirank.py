"""Global and CFL diagnostics over several ranks (tests/mr_gpu_diag.py): every global scalar, every CFL value and every address are
bit for bit those of the single-rank run; a maximum that ties belongs to the first cell in global block order on any distribution."""
import os

import pytest

from mr_launch import ROOT, run_check

pytestmark = pytest.mark.gpu


def test_two_ranks_equal_single_rank():
    run_check(["--nproc-per-node", "2", os.path.join(ROOT, "tests", "mr_gpu_diag.py"), "--config", "tiny", "--steps", "3",
               "--kw", "vmix_choice=3,km=24"], 300)
