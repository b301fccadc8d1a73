"""The northward heat and salt transports over several ranks (tests/mr_gpu_transport.py): every value of pop_transport_get and of
pop_transport_sums_get is, bit for bit and on every rank, that of the single-rank run of the same block decomposition."""
import os

import pytest

from mr_launch import ROOT, run_check

pytestmark = pytest.mark.gpu


def test_two_ranks_equal_single_rank():
    run_check(["--nproc-per-node", "2", os.path.join(ROOT, "tests", "mr_gpu_transport.py"), "--case", "gm_submeso", "--steps", "3"], 300)
