"""The N > 1 paths of rm_gather_frame / rm_gather_frame_root (csrc/rm_gather.hip) on the one GPU there is: the library
loads the loop-back stand-in tests/native/rccl_loopback.cpp instead of RCCL (RM_RCCL_LIBRARY) and one child process,
tests/loopback_gather_check.py, plays the ranks in turn.  Its docstring lists the cases and what each reaches: landing
slots of every rank (N = 2, 3, 4, 8; both plans), the send / receive pairing with empty ranks, the padded short shard,
landing-buffer reuse, the root's own copy, unaligned hit slots; and two deliberately wrong test-side sequences that
must come back as RM_E_RCCL at once.

What this cannot show: transport, xGMI, RCCL's own alignment or ordering behaviour, concurrency between ranks --
test_gpu_gather.py::test_two_rank_gather_over_rccl stays the test of the real exchange.

One child per group, one at a time, no retry.  The limit is over a WHOLE child -- interpreter start, the numpy import,
the dlopen of the library and rm_init included.  Measured on an MI355X: 0.60, 0.41 and 0.44 s for the three groups in a
first pass and 0.50, 0.39, 0.45 s in a second; the coldest ever seen, the first child on a machine that had not mapped the
library before, stayed under 0.9 s.  Five times that is 4.5 s, rounded up to 5 s per child."""
import os
import subprocess
import sys

import pytest

from loopback_stub import build_stub

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_SECONDS = 5


@pytest.fixture(scope="module")
def stub():
    return build_stub()


@pytest.mark.parametrize("group", ["cyclic", "contiguous", "reuse"])
def test_every_rank_of_a_gather_in_one_process(stub, group):
    """Bit-exact frames on every rank (all-gather) and on roots 0, N // 2, N - 1 (gather to root), untouched rows behind
    the frame, nothing left parked, the plan's call and byte counts; `reuse` adds the landing buffers across frames of
    changing size and the two negative checks, each followed by a green case in the same process."""
    env = dict(os.environ, RM_RCCL_LIBRARY=stub)
    env.pop("RM_HIP_LIB", None)
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.join(ROOT, "tests", "loopback_gather_check.py"), group]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=CHILD_SECONDS, env=env, cwd=ROOT)
    print(out.stdout)
    assert out.returncode == 0 and f"LOOPBACK_OK {group}" in out.stdout, (group, out.returncode, out.stdout[-3000:], out.stderr[-3000:])
    if group == "reuse":
        assert out.stdout.count("RM_E_RCCL") == 2, out.stdout[-3000:]
