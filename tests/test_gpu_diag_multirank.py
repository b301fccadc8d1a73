"""Global and CFL diagnostics over several ranks (tests/mr_gpu_diag.py): every global scalar, every CFL value and every address are
bit for bit those of the single-rank run; a maximum that ties belongs to the first cell in global block order on any distribution."""
import os

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_two_ranks_equal_single_rank():
    from test_gpu_multirank import _run_check
    _run_check(["--nproc-per-node", "2", os.path.join(ROOT, "tests", "mr_gpu_diag.py"), "--config", "tiny", "--steps", "3",
                "--kw", "vmix_choice=3,km=24"], 300)
