"""Every k_chain_run instance under wave skew, not only the 8-wave LDS-layout ones: the
skew build (mcmc-in-tonga_amd/libtdstar_skew.so, -DTD_CHAIN_SKEW) puts one wave to sleep for longer
than a phase after every block barrier and barrier-free phase end, so a shared word that no
synchronisation orders shows up as a state that differs from the reference's, or as a spin wait that gives
up.  tests/skew_instances_worker.py (a child process: the library is chosen at load) runs one case per
instance and run-time mode of the launcher's table (csrc/chain_kernels.hip kChainInstances) against the
HOST engine -- a full td_evaluate per proposal through kernels the skew build shares with the product --
and reports, with tdt_chain_launch_counts, which table entries its device launches took: a case that
quietly ran instance 0 again fails.  CASES names each case's target; judge() is the parent's whole
judgement of the worker's rows, held against made-up rows by tests/test_data_and_abi.py without a GPU."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SKEW = os.path.join(ROOT, "mcmc-in-tonga_amd", "libtdstar_skew.so")
WORKER = os.path.join(ROOT, "tests", "skew_instances_worker.py")

# case -> (its k_chain_run instance: the position in the launcher's table, the child process it runs in,
# the figures of its reference runs that must reach a minimum).  `accepted`: the least count of accepted
# proposals of any of the four actions in any of the case's twins; `swaps`: accepted swaps of the twin
# ladder; `long_shifts`: accepted deaths of the twin whose shift of the order in HBM takes more than one
# round of the block (8 x 512 entries, 8 x 256 in the 4-wave instances).
CASES = {
    "hbm_free": (2, "hbm", {"accepted": 1, "long_shifts": 2}),
    "hbm_rb": (2, "hbm", {"swaps": 1}),
    "rec_hbm": (9, "hbm", {"accepted": 1}),
    "packed_hbm": (4, "packed", {"accepted": 1, "long_shifts": 2}),
    "packed_tiles": (5, "packed", {"accepted": 1, "long_shifts": 2}),
    "rec_packed_hbm": (10, "packed", {"accepted": 1}),
    "rec_packed_tiles": (11, "packed", {"accepted": 1}),
    "dropin_lds": (1, "scripted", {"accepted": 1}),
    "dropin_hbm": (3, "scripted", {"accepted": 1}),
    "lds_rb": (0, "rounds", {"swaps": 1}),
    "xch_lds": (6, "rounds", {"swaps": 1}),
    "xch_hbm": (7, "rounds", {"swaps": 1}),
    "ladder_rec_hbm": (13, "rounds", {"swaps": 1}),
}
# the instances whose skew cases are the three older workers' (their tests' assertions are their own)
CREDITED = {0: "tests/skew_worker.py", 8: "tests/skew_history_worker.py", 12: "tests/skew_tempering_worker.py"}
# every instance that has a skew case: the launcher's table must be no longer than this
TARGETS = sorted(set(t for t, _, _ in CASES.values()) | set(CREDITED))


def group(name):
    return [c for c, (_, g, _) in CASES.items() if g == name]


def judge(rows, names):
    """What is wrong with the worker's rows for the cases `names`: [] when every case is there once, equals
    its reference, tripped no spin guard, launched its target instance at least once (and its reference no
    chain kernel at all) and met its conditions."""
    bad = []
    got = [r.get("case") for r in rows]
    for name in names:
        if got.count(name) != 1:
            bad.append("%s: %d rows" % (name, got.count(name)))
    for r in rows:
        name = r.get("case")
        if name not in names:
            bad.append("%r: not asked for" % (name,))
            continue
        target, _, need = CASES[name]
        if r.get("same") is not True:
            bad.append("%s: differs from its reference (%s)" % (name, r.get("why")))
        if r.get("guard") != 0:
            bad.append("%s: a spin wait gave up, guard %r, sites %r" % (name, r.get("guard"), r.get("sites")))
        launched = r.get("launched") or []
        if not (len(launched) > target and launched[target] >= 1):
            bad.append("%s: instance %d never launched (%r)" % (name, target, launched))
        if r.get("twin_launched") != 0:
            bad.append("%s: the reference launched a chain kernel (%r)" % (name, r.get("twin_launched")))
        for key, least in need.items():
            v = r.get(key)
            v = min(v) if isinstance(v, list) and v else v
            if not (isinstance(v, int) and v >= least):
                bad.append("%s: %s is %r, needs %d" % (name, key, r.get(key), least))
    return bad


def run_group(name, timeout):
    assert os.path.exists(SKEW), "the skew build is made by __graft_entry__.build() (make all)"
    names = group(name)
    env = dict(os.environ, TD_LIB_PATH=SKEW)
    p = subprocess.run([sys.executable, "-u", WORKER] + names, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=timeout, cwd=ROOT)
    text = p.stdout.decode(errors="replace")
    rows = [json.loads(x) for x in text.splitlines() if x.startswith("{")]
    assert p.returncode == 0, text[-3000:]
    assert judge(rows, names) == [], text[-3000:]


# Each child was timed once on an MI355X (the test's whole call, start of the child included); its subprocess
# limit is about four times that -- a cold first launch, a busy shared machine -- and pytest's a little above it.
@pytest.mark.gpu
@pytest.mark.timeout(14)
def test_hbm_layout_instances_under_wave_skew():
    """Instances 2 (free-running, and with host-decided resident rounds) and 9.  Measured: 2.2 s."""
    run_group("hbm", 9)


@pytest.mark.gpu
@pytest.mark.timeout(21)
def test_four_wave_instances_under_wave_skew():
    """Instances 4, 5, 10 and 11 (two chains per CU).  Measured: 3.8 s."""
    run_group("packed", 16)


@pytest.mark.gpu
@pytest.mark.timeout(12)
def test_scripted_instances_under_wave_skew():
    """Instances 1 and 3 (td_evaluate's resident server, and its launch per call).  Measured: 1.5 s."""
    run_group("scripted", 7)


@pytest.mark.gpu
@pytest.mark.timeout(10)
def test_round_instances_under_wave_skew():
    """Instances 0 with host-decided rounds, 6, 7 and 13.  Measured: 1.0 s."""
    run_group("rounds", 5)
