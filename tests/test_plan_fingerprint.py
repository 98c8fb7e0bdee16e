"""The planner's whole output, pinned: tools/sanitize/plan_fingerprint.cpp runs pack_problem and plan_kernels on a fixed list of
small descriptions and prints return codes, messages, the kernel choice and, as name:elements:hash, every table the driver reads.
tests/data/plan_fingerprint.txt is that text as printed by the planner before it was split into stages (the tool built with
-DPLAN_FINGERPRINT_BOOL_SWITCHES against that commit).  A change that MEANS to alter a table regenerates the file with the tool."""
import glob
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plan_fingerprint_matches_recorded_output(tmp_path):
    exe = str(tmp_path / "plan_fingerprint")
    sources = sorted(glob.glob(os.path.join(ROOT, "polydeal_amd", "csrc", "pdh_plan*.cpp")))
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-pthread", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "polydeal_amd", "csrc")] + sources +
                          [os.path.join(ROOT, "tools", "sanitize", "plan_fingerprint.cpp"), "-o", exe])
    env = {k: v for k, v in os.environ.items() if not k.startswith("PDH_")}
    got = subprocess.run([exe], check=True, capture_output=True, text=True, env=env).stdout.splitlines()
    with open(os.path.join(ROOT, "tests", "data", "plan_fingerprint.txt")) as f:
        want = f.read().splitlines()
    case = ""
    for i, (g, w) in enumerate(zip(got, want)):
        if w.startswith("=="):
            case = w
        fields = [x for x, y in zip(g.split(), w.split()) if x != y]
        assert g == w, "line %d differs (in %s) at %s: got %r, recorded %r" % (i + 1, case, fields[:1], g, w)
    assert len(got) == len(want), "the tool printed %d lines, %d are recorded" % (len(got), len(want))
