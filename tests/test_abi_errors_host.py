"""The error contract of the C ABI on a CPU: after a non-OK return aslr_last_error() describes THAT call -- the message starts
with the name of the function that refused and names what it refused -- whatever an earlier failure on the thread left
behind.  Every refusal here is decided before a device is touched, so no GPU is needed; a source check stands in for the
failing returns that only a device can reach."""
import ctypes as C
import os
import re

import pytest

from aslr_to_amd import _abi, scenarios

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ABI_SOURCE = os.path.join(ROOT, "aslr_to_amd", "csrc", "aslr_abi.hip")


def _last(lib):
    return lib.aslr_last_error().decode()


def _create(lib, desc):
    out = C.c_void_p()
    return lib.aslr_problem_create(C.byref(desc), None, 0, None, C.byref(out))


def test_a_failure_is_reported_with_its_own_cause_not_the_previous_one():
    lib = _abi.load_library()
    first = scenarios.lower(scenarios.two_dof_sea(B=2, T=3))
    first.desc.nmodels = 0
    assert _create(lib, first.desc) == _abi.E_INVALID
    msg1 = _last(lib)
    assert msg1.startswith("aslr_problem_create") and "nmodels" in msg1, msg1
    second = scenarios.lower(scenarios.two_dof_sea(B=2, T=3))
    second.desc.node_model = C.POINTER(C.c_int32)()
    assert _create(lib, second.desc) == _abi.E_INVALID
    msg2 = _last(lib)
    assert msg2.startswith("aslr_problem_create") and "node_model" in msg2, msg2
    assert msg1 not in msg2 and "nmodels = 0" not in msg2, msg2


def test_workspace_bytes_names_the_field_out_of_range():
    lib = _abi.load_library()
    low = scenarios.lower(scenarios.two_dof_sea(B=2, T=3))
    low.desc.chain.nj = 8
    assert lib.aslr_workspace_bytes(C.byref(low.desc)) < 0
    msg = _last(lib)
    assert msg.startswith("aslr_workspace_bytes") and "nj" in msg, msg


def test_residual_len_names_what_it_refuses():
    lib = _abi.load_library()
    low = scenarios.lower(scenarios.two_dof_sea(B=2, T=3))
    assert lib.aslr_residual_len(C.byref(low.desc.models[0]), 2) > 0
    assert lib.aslr_residual_len(C.byref(low.desc.models[0]), 0) == _abi.E_INVALID
    msg = _last(lib)
    assert msg.startswith("aslr_residual_len") and "nj" in msg, msg


# exports that take no handle (their refusals are tested above), and the one that accepts a NULL handle
NO_HANDLE = {"aslr_abi_version", "aslr_sizeof", "aslr_record_len", "aslr_solver_params_default", "aslr_workspace_bytes",
             "aslr_problem_create", "aslr_residual_len", "aslr_last_error"}
NULL_IS_NO_ERROR = {"aslr_problem_destroy"}   # like free(NULL)


def _null_handle_calls():
    """name -> the arguments behind the NULL handle: plausible ones, so that the handle is what is refused"""
    sp = _abi.default_solver_params(_abi.SOLVER_FDDP)
    psp = C.byref(sp)
    i32, f32, region = C.c_int32(), (C.c_float * 3)(), _abi.Region()
    tp, mpc, pool = _abi.TrajParams(), _abi.Mpc(n_steps=1, first_maxiter=1, iters_per_step=1), _abi.Pool(P=1)
    eye = (C.c_double * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
    zero3 = (C.c_double * 3)()
    buf = C.cast((C.c_double * 64)(), C.c_void_p)   # stands where a device pointer goes; never dereferenced
    keep = (sp, i32, f32, region, tp, mpc, pool, eye, zero3, buf)
    return keep, {
        "aslr_problem_region": (0, C.byref(region)),
        "aslr_calc": (None,), "aslr_calc_diff": (None,), "aslr_finalize": (None,),
        "aslr_backward_pass": (psp, None), "aslr_forward_pass": (psp, None),
        "aslr_solve": (psp, 4, None, C.byref(i32)),
        "aslr_iterate": (psp, 1, None), "aslr_iterate_n": (psp, 1, 2, None),
        "aslr_iterate_timed": (psp, 1, None, f32),
        "aslr_count_active": (None, C.byref(i32)),
        "aslr_dam_eval": (0, 1, buf, buf) + (None,) * 9 + (None,),
        "aslr_dam_residuals": (0, 1, buf, buf, buf, None),
        "aslr_quasi_static": (100, 1e-9, None, None),
        "aslr_frame_placement": (0, eye, zero3, 1, buf, 8, buf, None),
        "aslr_set_iteration_log": (buf, 4),
        "aslr_set_subshards": (2,),
        "aslr_solve_pool": (psp, C.byref(pool), 4, 16, None, C.byref(i32)),
        "aslr_set_trajectory_params": (C.byref(tp), None),
        "aslr_mpc_run": (psp, C.byref(mpc), None),
        "aslr_set_reference_path": (buf, 3, 0, None),
        "aslr_reference_row": (C.byref(i32),),
    }


def test_every_export_is_accounted_for():
    """A new export must either take no handle, or be given a NULL-handle call below."""
    assert set(_null_handle_calls()[1]) | NO_HANDLE | NULL_IS_NO_ERROR == set(_abi.EXPORTED_SYMBOLS)


@pytest.mark.parametrize("name", sorted(set(_abi.EXPORTED_SYMBOLS) - NO_HANDLE - NULL_IS_NO_ERROR))
def test_a_null_handle_is_refused_by_name(name):
    lib = _abi.load_library()
    assert lib.aslr_workspace_bytes(None) < 0     # some other message is in the buffer first
    assert _last(lib).startswith("aslr_workspace_bytes")
    keep, calls = _null_handle_calls()
    assert getattr(lib, name)(None, *calls[name]) == _abi.E_INVALID
    assert _last(lib).startswith(name + ":"), _last(lib)
    del keep


def test_destroying_a_null_handle_is_no_error():
    assert _abi.load_library().aslr_problem_destroy(None) == _abi.OK


def _host_code():
    """aslr_abi.hip without comments, preprocessor lines and string contents"""
    src = open(ABI_SOURCE).read()
    src = re.sub(r'"(?:\\.|[^"\\])*"|//[^\n]*', lambda m: '""' if m.group(0)[0] == '"' else "", src)
    return "\n".join(l for l in src.split("\n") if not l.lstrip().startswith("#"))


@pytest.mark.parametrize("code", ["ASLR_E_INVALID", "ASLR_E_HIP", "ASLR_E_NODEVICE", "ASLR_E_WORKSPACE"])
def test_no_error_code_leaves_the_abi_source_without_a_message(code):
    """Stands in for the failing returns a CPU cannot reach: in aslr_abi.hip an error code appears only as the first
    argument of fail(), which writes the message; nothing returns one bare or assigns one to a result."""
    src = _host_code()
    uses = [m.start() for m in re.finditer(r"\b%s\b" % code, src)]
    bare = [src[max(0, i - 40):i + len(code)] for i in uses if not re.search(r"\bfail\(\s*$", src[:i])]
    assert not bare, bare
    assert not re.search(r"return\s+ASLR_E_", src)


def test_hip_try_reports_through_fail():
    common = open(os.path.join(os.path.dirname(ABI_SOURCE), "aslr_common.hpp")).read()
    macro = common[common.index("#define HIP_TRY"):]
    macro = macro[:macro.index("while (0)")]
    assert "fail(ASLR_E_HIP" in macro and "snprintf" not in macro


def test_the_environment_is_read_in_one_place():
    assert len(re.findall(r"\bgetenv\b", _host_code())) == 1      # read_env alone reads the environment
