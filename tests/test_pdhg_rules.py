"""CPU tier: what a PDHG check decides (csrc/pdhg_check.hpp: pdhg_stop / pdhg_next), on scripted sequences of check sums.

tests/c/pdhg_rules.cpp is compiled against the header with the host compiler alone -- no HIP -- and run once; each case there is
written so that one rule fires, under the host loop's rule set and, for the exits, under the device-side loops' rule set.  The
expected exits, actions and values are literals worked out from the rule text of DESIGN.md section 5."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [
    "host_convergence", "host_stagnation_exit", "host_stalled_row_exit", "host_nan_residual",
    "device_convergence", "device_stagnation_exit", "device_stalled_row_exit", "device_nan_residual",
    "restart_sufficient", "restart_necessary", "restart_artificial",
    "backoff_flat_residual", "backoff_negative_r2", "backoff_growing_residual",
    "consolidation_trigger_and_cap", "consolidation_needs_flat_residual",
    "weight_update_and_clamp", "weight_damping",
]


def _clangxx():
    for c in ("/opt/rocm/lib/llvm/bin/clang++", "/opt/rocm/llvm/bin/clang++", shutil.which("clang++")):
        if c and os.path.exists(c):
            return c
    raise RuntimeError("no clang++ found (looked in the ROCm LLVM directories and on PATH)")


@pytest.fixture(scope="module")
def rules_output(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pdhg_rules") / "pdhg_rules")
    subprocess.run([_clangxx(), "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-O1",
                    "-I" + os.path.join(ROOT, "katana.jl_amd", "csrc"), os.path.join(ROOT, "tests", "c", "pdhg_rules.cpp"), "-o", exe],
                   check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    return r.returncode, r.stdout


@pytest.mark.parametrize("case", CASES)
def test_pdhg_rule(rules_output, case):
    _, out = rules_output
    lines = [ln for ln in out.split("\n") if ln.startswith("case %s " % case) or ln.startswith("  %s:" % case)]
    assert lines == ["case %s ok" % case], "\n".join(lines) or out


def test_every_case_of_the_program_is_listed_and_passes(rules_output):
    code, out = rules_output
    ran = [ln.split()[1] for ln in out.split("\n") if ln.startswith("case ")]
    assert sorted(ran) == sorted(CASES)
    assert code == 0 and out.strip().endswith("all ok"), out


def test_header_is_plain_cxx_without_hip():
    text = open(os.path.join(ROOT, "katana.jl_amd", "csrc", "pdhg_check.hpp")).read()
    includes = [ln for ln in text.split("\n") if ln.startswith("#include")]
    assert includes == ["#include <cmath>"], includes
