"""Time-averaged output over several ranks (tests/mr_gpu_tavg.py): every rank's buffers of TEMP, KE, SSH, HBLT, TEMP_MAX and RHO_VINT
and the sums of both streams are bit for bit those of the single-rank run, ghost cells included, and the tavg file the ranks write
together equals the single-rank file byte for byte, header included."""
import os

import pytest

from mr_launch import ROOT, run_check

pytestmark = pytest.mark.gpu


def test_two_ranks_equal_single_rank():
    run_check(["--nproc-per-node", "2", os.path.join(ROOT, "tests", "mr_gpu_tavg.py"), "--config", "tiny", "--steps", "3",
               "--kw", "vmix_choice=3,km=24"], 300)
