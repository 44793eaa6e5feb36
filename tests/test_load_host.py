"""CPU tier: the index arithmetic of loadproblem (csrc/load_host.hpp) -- the blocked and the batched copy of the NL entries, the shape
classes of the tape rows, postfix_to_nodes, the bound-box vertex and the epigraph cut there -- on the smallest inputs that reach
each branch.

tests/c/load_host.cpp is compiled against the header with the host compiler alone -- no HIP -- under AddressSanitizer and UBSan
(-fno-sanitize-recover=all: any report ends the program) and run once.  Nothing is preloaded and no GPU is touched; like the host
ASan harness of the ABI layer (test_abi.py) the test keeps to the CPU tier and skips where a GPU device node is present."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [
    "blocked_entries_once_in_segment", "blocked_kinds_grouped_stable", "blocked_tape_row_empty", "blocked_bseg_scan",
    "batched_entries_in_buckets", "batched_rows_ascend", "batched_segs_scan",
    "classify_constants_share_a_class", "classify_powc_exponent_splits", "classify_nl_row_splits", "classify_structure_length_splits",
    "postfix_duplicate_column_first_slot", "postfix_binary_underflow", "postfix_stack_not_reduced", "postfix_var_missing_from_row",
    "postfix_var_beyond_the_columns", "postfix_unknown_opcode",
    "vertex_smaller_magnitude_and_tie", "vertex_infinite_sides", "vertex_crossed_bounds_clear_ok",
    "cut_nan_coefficient_not_finite", "cut_pad_zero_lifts_maximum", "cut_rounding_threshold", "cut_constant",
]


def _clangxx():
    for c in ("/opt/rocm/lib/llvm/bin/clang++", "/opt/rocm/llvm/bin/clang++", shutil.which("clang++")):
        if c and os.path.exists(c):
            return c
    raise RuntimeError("no clang++ found (looked in the ROCm LLVM directories and on PATH)")


@pytest.fixture(scope="module")
def load_host_output(tmp_path_factory):
    if os.path.exists("/dev/kfd"):
        pytest.skip("sanitizer builds run on the CPU tier only (a GPU device node is present)")
    exe = str(tmp_path_factory.mktemp("load_host") / "load_host")
    subprocess.run([_clangxx(), "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    "-I" + os.path.join(ROOT, "katana.jl_amd", "csrc"), os.path.join(ROOT, "tests", "c", "load_host.cpp"), "-o", exe],
                   check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    return r.returncode, r.stdout, r.stderr


@pytest.mark.parametrize("case", CASES)
def test_load_host(load_host_output, case):
    _, out, err = load_host_output
    lines = [ln for ln in out.split("\n") if ln.startswith("case %s " % case) or ln.startswith("  %s:" % case)]
    assert lines == ["case %s ok" % case], "\n".join(lines) or out + err[-3000:]


def test_every_case_of_the_program_is_listed_and_no_sanitizer_reports(load_host_output):
    code, out, err = load_host_output
    ran = [ln.split()[1] for ln in out.split("\n") if ln.startswith("case ")]
    assert sorted(ran) == sorted(CASES)
    assert code == 0 and out.strip().endswith("all ok"), out + err[-3000:]
    assert "Sanitizer" not in err and "runtime error" not in err, err[-3000:]


def test_header_is_plain_cxx_without_hip():
    csrc = os.path.join(ROOT, "katana.jl_amd", "csrc")
    for name in ("load_host.hpp", "error.hpp"):
        for ln in open(os.path.join(csrc, name)).read().split("\n"):
            if ln.startswith("#include"):
                assert ln.startswith("#include <") and "hip" not in ln or ln in ('#include "error.hpp"', '#include "../../include/katana_hip.h"'), ln
