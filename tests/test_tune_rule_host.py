"""The decision rule of the spectrum audition (biahub_amd/csrc/tune_rule.hpp) on a host, without a GPU: a stand-alone C++
program (tests/tune_rule_host.cpp, its own main, the host compiler, UBSan) feeds it timing sequences one draw at a time, as
fftconv_tune_spectrum does, and reports where the rule stopped and which candidate it kept."""

import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent

# case -> (number of candidates drawn when the rule said stop, 0 = it never did; index kept).  Rule of the cases: K = 5, two
# levels when fastest < 0.9 * slowest.
EXPECTED = {
    "one_candidate_only": (1, 0),   # K = 1: the caller's allocation, no draw
    "one_of_five": (0, 0),          # one time says nothing yet: continue
    "all_equal": (5, 0),            # K reached, the earliest of equals stays
    "fast_first": (2, 0),           # 6.0 then 6.9: both levels seen after one draw, the first stays
    "slow_slow_fast": (3, 2),       # 6.9, 7.0 are one level; 6.0 is the second: stop there and keep it
    "k_reached_one_level": (5, 3),  # 6.00-6.20: never two levels, the fastest of K stays
    "just_above_ratio": (5, 1),     # 9.1 / 10 is above 0.9: one level
    "failed_second": (2, 0),        # a candidate without a time ends the draws; the timed one stays
    "failed_after_better": (3, 1),  # ... and the best so far is a drawn one
    "failed_first": (1, 0),         # nothing has a time: the caller's allocation stays
}


@pytest.fixture(scope="module")
def rule_output(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path_factory.mktemp("tune_rule") / "tune_rule_host"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=undefined", "-fno-sanitize-recover=all",
                    f"-I{ROOT / 'biahub_amd' / 'csrc'}", str(ROOT / "tests" / "tune_rule_host.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


@pytest.mark.parametrize("case", sorted(EXPECTED))
def test_rule_stop_point_and_index_kept(rule_output, case):
    got = {}
    for line in rule_output.splitlines():
        w = line.split()
        if len(w) == 5 and w[1] == "stop" and w[3] == "keep":
            got[w[0]] = (int(w[2]), int(w[4]))
    assert set(got) == set(EXPECTED)
    assert got[case] == EXPECTED[case]


def test_default_rule_is_a_rule(rule_output):
    w = [ln.split() for ln in rule_output.splitlines() if ln.startswith("default ")][0]
    k, ratio = int(w[2]), float(w[4])
    assert 1 <= k <= 16 and 0.5 < ratio < 1.0


def test_rule_header_has_no_hip_in_it():
    text = (ROOT / "biahub_amd" / "csrc" / "tune_rule.hpp").read_text()
    assert "#include" not in text and "__global__" not in text and "hipError" not in text
