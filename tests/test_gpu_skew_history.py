"""The recorded chain launch under wave skew (the mechanism of test_gpu_skew.py: the skew build,
mcmc-in-tonga_amd/libtdstar_skew.so, sleeps one wave for longer than a phase after every block barrier,
the sample copy's included).  td_chain_run_recorded with every 1 and every 3 on the 8-cell model at
max_cells 12 and on the 200-cell model must leave the history the HOST engine records from its host
loop, bit for bit, and no spin wait may give up (guard slot 0)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SKEW = os.path.join(ROOT, "mcmc-in-tonga_amd", "libtdstar_skew.so")


@pytest.mark.timeout(120)
def test_recorded_chain_follows_host_under_wave_skew():
    assert os.path.exists(SKEW), "the skew build is made by __graft_entry__.build() (make all)"
    env = dict(os.environ, TD_LIB_PATH=SKEW)
    p = subprocess.run([sys.executable, "-u", os.path.join(ROOT, "tests", "skew_history_worker.py")], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=110, cwd=ROOT)
    text = p.stdout.decode(errors="replace")
    rows = [json.loads(x) for x in text.splitlines() if x.startswith("{")]
    assert p.returncode == 0 and len(rows) == 4, text[-3000:]
    assert all(r["same"] and r["end"] and r["guard"] == 0 and r["samples"] > 0 for r in rows), rows
    assert {(r["cells"], r["every"]) for r in rows} == {(8, 1), (8, 3), (200, 1), (200, 3)}
