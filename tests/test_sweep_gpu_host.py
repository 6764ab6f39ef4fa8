"""The shared bodies of tests/_sweep_gpu.py on a CPU: they stand in three GPU suites at once, and one that cannot fail would
disarm all three.  A fake call returns numpy arrays at B = 3, T = 2, nx = 8; every body passes on consistent data and raises
on data that is wrong in one place: an output off by a relative 1e-8 on one trajectory, a wrong shape, an output made alone
that differs in its last bit, a variance on a zero gain row, a padded control that is not zero.

trajectory_alone, side_effects_of_calc_diff and the two facade bodies need an engine: the GPU suites are their only cover."""
import numpy as np
import pytest

import _sweep_gpu as sw

B, T, NX, NU = 3, 2, 8, 2
FIELDS = ("x_var", "u_var", "cost_increase")


def _outputs():
    """batch-major outputs of a sweep: fresh arrays, the same values every time"""
    rng = np.random.default_rng(5)
    return {"x_var": rng.uniform(0.1, 1.0, (B, T + 1, NX)), "u_var": rng.uniform(0.1, 1.0, (B, T, NU)),
            "cost_increase": rng.uniform(0.1, 1.0, (B,))}


def _call(which=FIELDS):
    full = _outputs()
    return {k: full[k] for k in which}


def _gains():
    """K [T, B, nu, nx] with two zero rows"""
    K = np.random.default_rng(6).uniform(0.5, 1.0, (T, B, NU, NX))
    K[0, 1, 1] = 0.0
    K[1, 2, 0] = 0.0
    return K


def _zeroed(K):
    """the outputs with u_var zero on the zero rows of K"""
    got = _outputs()
    got["u_var"].transpose(1, 0, 2)[np.abs(K).max(axis=-1) == 0.0] = 0.0
    return got


def test_matches_passes_on_a_copy():
    sw.matches(_call(), _outputs(), FIELDS, "copy")


@pytest.mark.parametrize("field", FIELDS)
def test_matches_raises_on_a_relative_1e_8_on_one_trajectory(field):
    got = _call()
    got[field][1] *= 1.0 + 1e-8
    with pytest.raises(AssertionError, match=field):
        sw.matches(got, _outputs(), FIELDS, "off")
    sw.matches(got, _outputs(), [k for k in FIELDS if k != field], "the others")


def test_matches_raises_on_a_wrong_shape():
    got = _call()
    got["x_var"] = got["x_var"][:, :-1]
    with pytest.raises(AssertionError, match="x_var"):
        sw.matches(got, _outputs(), FIELDS, "short")


def test_each_output_alone_passes_on_the_same_bits():
    sw.each_output_alone(_call, _call())


@pytest.mark.parametrize("field", FIELDS)
def test_each_output_alone_raises_on_a_last_bit(field):
    full = _call()
    last = full[field].reshape(-1)[-1:]
    last[:] = np.nextafter(last, 2.0)
    with pytest.raises(AssertionError, match=field):
        sw.each_output_alone(_call, full)


def test_each_output_alone_raises_when_the_call_returns_another_output_too():
    with pytest.raises(AssertionError, match="keys"):
        sw.each_output_alone(lambda which: _call(), _call())


def test_zero_gain_rows():
    K = _gains()
    sw.zero_gain_rows("vsa_box", K, _zeroed(K))
    sw.zero_gain_rows("sea", K, _outputs())   # (no BoxDDP gains: nothing is asked)
    for key in ("vsa_box", "arm_vsa"):
        with pytest.raises(AssertionError):
            sw.zero_gain_rows(key, K, _outputs())   # a variance on every zero row
    got = _zeroed(K)
    got["u_var"][2, 1, 0] = 1e-300   # ... on one of them
    with pytest.raises(AssertionError):
        sw.zero_gain_rows("vsa_box", K, got)
    for bad in (np.ones_like(K), np.zeros_like(K)):   # no zero row; nothing but zero rows
        with pytest.raises(AssertionError):
            sw.zero_gain_rows("vsa_box", bad, _zeroed(bad))


def test_padded_control():
    got = _outputs()
    sw.padded_control("sea", got)   # (no padded control: nothing is asked)
    with pytest.raises(AssertionError):
        sw.padded_control("nu1", got)
    got["u_var"][..., 1] = 0.0
    sw.padded_control("nu1", got)
    got["u_var"][1, 1, 1] = 1e-300
    with pytest.raises(AssertionError):
        sw.padded_control("nu1", got)
