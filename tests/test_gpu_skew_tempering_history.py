"""A recorded ladder's synchronisation under wave skew: the skew build (mcmc-in-tonga_amd/libtdstar_skew.so,
-DTD_CHAIN_SKEW) puts one wave to sleep for longer than a phase after every block barrier -- the one that
follows a round's sample included -- so a latch or a copy that a barrier does not order shows up as a
history that differs from the twin's, or as a spin wait that gives up.  Both round protocols must still
leave the twin's history (tests/skew_tempering_worker.py, a child process: the library is chosen at load)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SKEW = os.path.join(ROOT, "mcmc-in-tonga_amd", "libtdstar_skew.so")


@pytest.mark.timeout(120)
def test_recorded_ladder_equals_its_twin_under_wave_skew():
    assert os.path.exists(SKEW), "the skew build is made by __graft_entry__.build() (make all)"
    env = dict(os.environ, TD_LIB_PATH=SKEW)
    p = subprocess.run([sys.executable, "-u", os.path.join(ROOT, "tests", "skew_tempering_worker.py")], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=100, cwd=ROOT)
    text = p.stdout.decode(errors="replace")
    rows = [json.loads(x) for x in text.splitlines() if x.startswith("{")]
    assert p.returncode == 0 and [r["protocol"] for r in rows] == ["host", "device"], text[-3000:]
    assert all(r["same"] and r["trace"] and r["guard"] == 0 and r["samples"] == 11 for r in rows), rows
