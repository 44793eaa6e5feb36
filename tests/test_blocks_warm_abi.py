"""CPU tier: the surface of the warm re-solve of a resident batch (KTN_BLOCKS_WARM, ktn_blocks_rewarm; DESIGN.md section 14 "In the
device-side loop") through every layer that runs without a GPU -- the header, the library's export table, the Python and Julia
bindings and the front ends.  The solves are in tests/test_gpu_blocks_warm.py."""
import ctypes
import inspect
import os
import re

import katana_jl_amd as ktn
from katana_jl_amd import _lib as L
from katana_jl_amd.batch import FusedBatch
from katana_jl_amd.solver import KatanaNonlinearModel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "katana_hip.h")).read()
JL = open(os.path.join(ROOT, "katana.jl_amd", "julia", "KatanaHIP.jl")).read()
STATS = ("ecp_blocks_warm_launches", "ecp_blocks_warm_instances", "ecp_blocks_warm_cold_instances", "ecp_blocks_warm_infeasible",
         "ecp_blocks_warm_dropped_rows", "ecp_blocks_warm_clamped_cols")


def test_header_defines_the_flag_and_declares_the_entry_point():
    m = re.search(r"^#define\s+KTN_BLOCKS_WARM\s+\(?(\d+)\)?", HEADER, re.M)
    assert m and int(m.group(1)) == 4
    assert re.search(r"\bint ktn_blocks_rewarm\(ktn_handle h, double\* out, int64_t cap, int64_t\* count\);", HEADER)
    assert re.search(r"#define\s+KTN_ABI_VERSION\s+1\b", HEADER)                  # the change only adds an entry point and a flag
    for stat in STATS:
        assert '"%s"' % stat in HEADER, stat
    # what a caller has to know stands where the flag and the entry point are declared
    doc = HEADER[HEADER.index("KTN_BLOCKS_WARM         re-solve"):HEADER.index("int ktn_blocks_get_results")]
    for word in ("k_blocks_rewarm", ":Infeasible", "0 PDHG iterations", "cold launch, bit for bit", "ecp_blocks_fallbacks", "KTN_BLOCKS_NO_FALLBACK"):
        assert word in doc, word
    doc = HEADER[HEADER.index("What has to happen between two device launches"):HEADER.index("int ktn_blocks_rewarm")]
    for word in ("state", "clamped", "crossed", "proving row", "redundant", "amin_k", "tau_k", "purge_margin", "M - m_lin > (cap_rows - m_lin) / 2",
                 "Idempotent", "KTN_E_INVALID"):
        assert word in doc, word
    # the setters' text no longer says that the device loop always starts cold
    setters = HEADER[HEADER.index("re-solve after a change of variable bounds"):HEADER.index("ktn_set_var_bounds: n == num_var")]
    assert "KTN_BLOCKS_WARM" in setters


def test_python_binding_and_library_carry_them():
    assert L.BLOCKS_WARM == 4 and (L.BLOCKS_SUPPORTING, L.BLOCKS_NO_FALLBACK) == (1, 2)
    assert L.PROTOTYPES["ktn_blocks_rewarm"] == (L.c_i32, [ctypes.c_void_p, L.P(L.c_f64), L.c_i64, L.P(L.c_i64)])
    lib = L.lib()
    raw = ctypes.CDLL(L.LIB_PATH)
    assert getattr(lib, "ktn_blocks_rewarm") is not None and hasattr(raw, "ktn_blocks_rewarm")      # exported
    assert lib.ktn_abi_version() == 1
    assert lib.ktn_blocks_rewarm(ctypes.c_void_p(), None, 0, None) == L.E_INVALID                   # a null handle is refused, not dereferenced


def test_params_and_description_did_not_grow():
    assert ctypes.sizeof(L.KtnParams) == L.lib().ktn_sizeof_params()
    assert ctypes.sizeof(L.KtnNlpDesc) == L.lib().ktn_sizeof_nlp_desc()
    assert not any("blocks" in f or "rewarm" in f for f, _ in L.KtnParams._fields_)      # the switch is a flag of the call, not a parameter


def test_julia_binding_has_the_constant_the_keyword_and_the_call():
    assert re.search(r"^const KTN_BLOCKS_WARM = 4$", JL, re.M)
    assert re.search(r"ccall\(\(:ktn_blocks_rewarm, LIB\), Cint,", JL)
    assert re.search(r"ccall\(\(:ktn_optimize_blocks_ex, LIB\), Cint,", JL)
    sig = re.search(r"^function optimize_blocks!\(m::KatanaHipModel;(.*)\)$", JL, re.M)
    assert sig and re.search(r"\bwarm = false\b", sig.group(1))
    assert re.search(r"warm \? KTN_BLOCKS_WARM : 0", JL)
    assert re.search(r"^export .*\boptimize_blocks!", JL, re.M) and re.search(r"^export .*\bblocks_rewarm\b", JL, re.M)


class _Recorder:
    """stands in for the loaded library: records which symbol a call went to"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name,) + tuple(a for a in args[1:]))
            return L.STATUS_OPTIMAL
        return fn


def test_front_ends_have_the_keyword_and_it_reaches_the_flag():
    assert inspect.signature(KatanaNonlinearModel.optimize_blocks).parameters["warm"].default is False
    assert inspect.signature(FusedBatch.solve).parameters["warm"].default is False
    assert callable(KatanaNonlinearModel.blocks_rewarm) and callable(ktn.LinearQuadraticModel.blocks_rewarm)
    m = object.__new__(KatanaNonlinearModel)                       # no handle: nothing below reaches the engine
    m._lib, m._h = _Recorder(), None
    m.optimize_blocks()
    m.optimize_blocks(warm=True)
    m.optimize_blocks(5, supporting=True, fallback=False, warm=True)
    assert m._lib.calls == [("ktn_optimize_blocks", 0), ("ktn_optimize_blocks_ex", 0, L.BLOCKS_WARM),
                            ("ktn_optimize_blocks_ex", 5, L.BLOCKS_SUPPORTING | L.BLOCKS_NO_FALLBACK | L.BLOCKS_WARM)]


def test_a_warm_solve_of_a_fused_batch_does_not_reset_the_handle():
    class _Model:
        def __init__(self):
            self.calls = []
            self.params = type("P", (), {"cut_algo": 0})()

        def reset(self):
            self.calls.append("reset")

        def optimize_blocks(self, cut_capacity, supporting, fallback, warm):
            self.calls.append(("optimize_blocks", cut_capacity, supporting, fallback, warm))
            raise _Stop()

    class _Stop(Exception):
        pass
    for warm, want in ((True, [("optimize_blocks", 0, False, True, True)]), (False, ["reset", ("optimize_blocks", 0, False, True, False)])):
        fb = object.__new__(FusedBatch)                            # a loaded, once-solved batch without its handle
        fb.m, fb.big, fb.offs, fb.device_loop, fb._solved = _Model(), None, [0, 1], True, True
        try:
            fb.solve(warm=warm)
        except _Stop:
            pass
        assert fb.m.calls == want, (warm, fb.m.calls)
