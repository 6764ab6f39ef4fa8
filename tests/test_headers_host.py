"""The ctypes binding (aslr_to_amd/_abi.py: PROTOTYPES and the *_SYMBOLS lists derived from it) against the headers under
include/ and the built library, on a CPU: one case per header, with the header's own text as the reference (tests/_headers.py),
and the facts about single prototypes that the per-extension host tests used to assert beside their copy of this check."""
import ctypes as C
import subprocess

import pytest

import _headers as H
from aslr_to_amd import _abi

HEADERS = list(_abi.PROTOTYPES)


def _defined():
    nm = subprocess.run(["nm", "-D", "--defined-only", _abi.lib_path()], capture_output=True, text=True, check=True).stdout
    return {l.split()[-1] for l in nm.splitlines() if l.split()[-2:-1] == ["T"]}


def test_the_table_has_a_row_and_a_list_for_every_header():
    assert HEADERS[0] == "aslr_to_amd.h" and sorted(HEADERS) == H.headers()
    assert list(_abi.SYMBOL_LISTS) == HEADERS and len(set(_abi.SYMBOL_LISTS.values())) == len(HEADERS)
    assert _abi.SYMBOL_LISTS["aslr_to_amd.h"] == "EXPORTED_SYMBOLS" and _abi.SYMBOL_LISTS["aslr_to_amd_sens.h"] == "EXTENSION_SYMBOLS"


@pytest.mark.parametrize("header", HEADERS)
def test_the_header_is_bound_and_exported(header):
    """The header declares exactly its symbol list; no other list and no other header knows one of its names (every pair of
    lists is met once from either side over the cases); the library defines every name and the binding has it, with as many
    argtypes as the declaration has parameters (unset only where it has none)."""
    names = getattr(_abi, _abi.SYMBOL_LISTS[header])
    declared = H.declared(header)
    assert declared and names == list(_abi.PROTOTYPES[header]) and len(names) == len(declared) and set(names) == declared
    for other in HEADERS:
        if other != header:
            assert not declared & set(getattr(_abi, _abi.SYMBOL_LISTS[other])), other
            assert not declared & H.declared(other), other
    assert declared <= _defined(), declared - _defined()
    lib = _abi.load_library()
    counts = H.parameter_counts(header)
    for name in names:
        f = getattr(lib, name)
        assert f.restype is _abi.PROTOTYPES[header][name][0], name
        assert (f.argtypes is None and counts[name] == 0) or len(f.argtypes) == counts[name], (name, counts[name])
        assert header == "aslr_to_amd.h" or (f.restype is C.c_int and f.argtypes is not None), name


def test_the_parameter_count_reads_a_declaration():
    """the reference of the argtypes check on the declarations whose counts the per-extension tests had written out by hand"""
    want = {"aslr_policy_rollout_all": 13, "aslr_mpc_run_plant_all": 10, "aslr_policy_rollout_noise": 20,
            "aslr_policy_plant_sensitivity": 12, "aslr_solve_pool_params": 8, "aslr_design_descent": 4, "aslr_plant_identify": 3,
            "aslr_abi_version": 0, "aslr_last_error": 0}
    got = {}
    for header in HEADERS:
        got.update(H.parameter_counts(header))
    assert {k: got[k] for k in want} == want


def test_single_prototypes():
    """the seed of the noise roll-out is a 64-bit word; the entry points for every model size take what their two-joint
    twins take (the struct of the pool parameters: tests/test_pool_params_host.py)"""
    lib = _abi.load_library()
    assert lib.aslr_policy_rollout_noise.argtypes[4] is C.c_uint64
    assert list(lib.aslr_policy_rollout_all.argtypes) == list(lib.aslr_policy_rollout.argtypes)
    assert list(lib.aslr_mpc_run_plant_all.argtypes) == list(lib.aslr_mpc_run_plant.argtypes)


def test_the_extensions_left_the_base_abi_alone():
    """ABI version 5, no struct index past 8, the ctypes mirrors of the structs the extension headers define, and the debug
    exports of the library in no header and in no list"""
    lib = _abi.load_library()
    assert _abi.ABI_VERSION == 5 and lib.aslr_abi_version() == 5
    assert lib.aslr_sizeof(9) == -1
    assert C.sizeof(_abi.Design) == 6 * 4 + 5 * 8 + 12 * C.sizeof(C.c_void_p)
    assert C.sizeof(_abi.Identify) == 4 * 4 + 7 * 8 + 14 * C.sizeof(C.c_void_p)
    debug = {n for n in _defined() if n.startswith("aslr_debug_")}
    assert {"aslr_debug_identify_step", "aslr_debug_identify_normal"} <= debug
    for header in HEADERS:
        assert not debug & H.declared(header) and not debug & set(_abi.PROTOTYPES[header]), header
