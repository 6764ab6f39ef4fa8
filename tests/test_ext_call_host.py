"""tests/_ext_call.py on the CPU: the checks the GPU suites of the extension calls lean on are themselves known to fire.  No
GPU, no call into the library: CPU tensors and plain integers for the return codes."""
import numpy as np
import pytest
import torch

import _ext_call as ext
import _gpu_case as gc

OK, REFUSED = 0, 3   # (any two distinct codes with OK = 0, the library's ASLR_OK)


def test_constants():
    assert (ext.GUARD, ext.SENTINEL, ext.SENTINEL_I32) == (64, -7.25, -7)
    assert OK == ext._abi.OK


@pytest.mark.parametrize("int32", [False, True])
@pytest.mark.parametrize("shape, perm", [((2, 3, 4), (1, 0, 2)), ((5,), None), ((3, 2), (1, 0)), ((0, 4), (1, 0)), ((), None)])
def test_a_fresh_buffer(shape, perm, int32):
    buf = ext.alloc(shape, "cpu", int32)
    n = int(np.prod(shape))
    assert buf.dtype == (torch.int32 if int32 else torch.float64) and tuple(buf.shape) == (n + ext.GUARD,)
    assert ext.untouched(buf) and ext.guard_intact(buf)
    a = ext.payload(buf, shape, perm)
    assert a.dtype == (np.int32 if int32 else np.float64)
    assert a.shape == (tuple(shape) if perm is None else tuple(shape[p] for p in perm))
    assert a.flags["C_CONTIGUOUS"] and (a == (ext.SENTINEL_I32 if int32 else ext.SENTINEL)).all()


def test_the_payload_is_cut_reshaped_and_transposed():
    shape = (2, 3, 4)
    buf = ext.alloc(shape, "cpu")
    buf[:24] = torch.arange(24, dtype=torch.float64)
    want = np.arange(24.0).reshape(shape)
    np.testing.assert_array_equal(ext.payload(buf, shape), want)
    np.testing.assert_array_equal(ext.payload(buf, shape, (1, 0, 2)), want.transpose(1, 0, 2))
    a = ext.payload(buf, shape)
    a[0, 0, 0] = 99.0   # an owned copy
    assert float(buf[0]) == 0.0


@pytest.mark.parametrize("int32", [False, True])
@pytest.mark.parametrize("word", [0, 5])
def test_one_payload_word_written(word, int32):
    buf = ext.alloc((2, 3), "cpu", int32)
    buf[word] = 1
    assert not ext.untouched(buf)
    assert ext.guard_intact(buf)


@pytest.mark.parametrize("int32", [False, True])
@pytest.mark.parametrize("word", [0, ext.GUARD - 1])
def test_one_guard_word_written(word, int32):
    """the first and the last guard word.  The known limit: a write of a value that EQUALS the sentinel is not seen, which is
    why the sentinels are -7.25 and -7, values no kernel here produces, and not 0"""
    buf = ext.alloc((2, 3), "cpu", int32)
    buf[6 + word] = 0
    assert not ext.guard_intact(buf) and not ext.untouched(buf)
    buf[6 + word] = ext.SENTINEL_I32 if int32 else ext.SENTINEL
    assert ext.guard_intact(buf) and ext.untouched(buf)   # the limit
    empty = ext.alloc((0,), "cpu", int32)                 # no payload: every word is guard
    empty[word] = 0
    assert not ext.guard_intact(empty)


def _nan(payload_bits):
    return np.array([0x7FF8000000000000 | payload_bits], dtype=np.uint64).view(np.float64)


def test_same_on_arrays():
    a = np.array([[1.0, -2.5], [0.0, 3.0]])
    ext.same(a, a.copy(), "equal")
    ext.same(a.T, np.ascontiguousarray(a.T), "a view that is not contiguous")
    with pytest.raises(AssertionError, match="signed zero"):
        ext.same(np.array([0.0]), np.array([-0.0]), "signed zero")
    ext.same(_nan(1), _nan(1), "the same NaN")
    with pytest.raises(AssertionError, match="two NaNs"):
        ext.same(_nan(1), _nan(2), "two NaNs")
    ext.same(np.array([1, -7], dtype=np.int32), np.array([1, -7], dtype=np.int32), "int32")
    with pytest.raises(AssertionError, match="int32 by value"):
        ext.same(np.array([1, -7], dtype=np.int32), np.array([1, 7], dtype=np.int32), "int32 by value")
    with pytest.raises(AssertionError, match="shapes"):
        ext.same(np.zeros(3), np.zeros(4), "shapes")


def test_same_on_dicts_and_none():
    a = dict(x=np.array([1.0, 2.0]), f=np.array([3], dtype=np.int32), c=None)
    ext.same(a, dict(a), "equal dicts")
    ext.same(None, None, "None on both sides")
    for one, other in ((None, np.zeros(2)), (np.zeros(2), None)):
        with pytest.raises(AssertionError, match="one side"):
            ext.same(one, other, "one side")
    with pytest.raises(AssertionError, match="the run: c"):
        ext.same(a, dict(a, c=np.zeros(1)), "the run")
    with pytest.raises(AssertionError, match="the run: the keys differ"):
        ext.same(a, {k: a[k] for k in ("x", "f")}, "the run")
    with pytest.raises(AssertionError, match="the run: the keys differ"):
        ext.same({k: a[k] for k in ("x", "f")}, a, "the run")
    with pytest.raises(AssertionError, match="the run: the keys differ"):
        ext.same(a, a["x"], "the run")
    with pytest.raises(AssertionError, match="the run: x"):
        ext.same(a, dict(a, x=np.array([1.0, -2.0])), "the run")


def test_relerr():
    assert gc.relerr(np.zeros((0, 3)), np.zeros((0, 3))) == 0.0
    # max(|1 - 1| / (1 + 1), |3 - 1| / (1 + 1), |-7 - -3| / (1 + 3)) = max(0, 1, 1), and a smaller one: 0.5 / (1 + 4)
    assert gc.relerr([1.0, 3.0, -7.0], [1.0, 1.0, -3.0]) == 1.0
    assert gc.relerr([4.5], [4.0]) == 0.5 / 5.0
    import _policy
    import _sensitivity
    assert _policy.relerr is gc.relerr and _sensitivity.relerr is gc.relerr


def _outs():
    return ext.outputs("cpu", {"cost": (3, 2), "failed_knot": (3, 2), "xs": (3, 4, 2)}, ("cost", "failed_knot"), perms={"cost": (1, 0)},
                      int32=("failed_knot",))


def test_outputs():
    outs = _outs()
    assert sorted(outs) == ["cost", "failed_knot"]
    assert outs["cost"].buf.dtype == torch.float64 and outs["failed_knot"].buf.dtype == torch.int32
    assert outs["cost"].perm == (1, 0) and outs["failed_knot"].perm is None and outs["cost"].shape == (3, 2)
    assert ext.ptr(None) is None and ext.ptr(outs["cost"]).value == outs["cost"].buf.data_ptr() == ext.ptr(outs["cost"].buf).value


def test_a_success_returns_the_payloads():
    outs = _outs()
    outs["cost"].buf[:6] = torch.arange(6, dtype=torch.float64)
    outs["failed_knot"].buf[:6] = -1
    got = ext.conclude(OK, OK, outs, "")
    assert sorted(got) == ["cost", "failed_knot"]
    np.testing.assert_array_equal(got["cost"], np.arange(6.0).reshape(3, 2).T)
    assert got["failed_knot"].dtype == np.int32 and got["failed_knot"].shape == (3, 2) and (got["failed_knot"] == -1).all()


def test_a_success_with_a_touched_guard_fails():
    for k in ("cost", "failed_knot"):
        outs = _outs()
        outs[k].buf[6] = 0
        with pytest.raises(AssertionError, match="guard behind %s .* aslr_x" % k):
            ext.conclude(OK, OK, outs, "", "aslr_x")


def test_a_refusal_that_wrote_nothing_returns_the_message():
    assert ext.conclude(REFUSED, REFUSED, _outs(), "aslr_x: no") == "aslr_x: no"
    assert ext.conclude(REFUSED, REFUSED, {}, "aslr_x: every output NULL") == "aslr_x: every output NULL"


def test_a_refusal_that_wrote_a_word_fails():
    for k, word in (("cost", 0), ("failed_knot", 5), ("cost", 6 + ext.GUARD - 1)):
        outs = _outs()
        outs[k].buf[word] = 0
        with pytest.raises(AssertionError, match="%s was written by the refused aslr_x" % k):
            ext.conclude(REFUSED, REFUSED, outs, "aslr_x: no", "aslr_x")


def test_an_unexpected_return_code_fails():
    with pytest.raises(AssertionError, match="aslr_x returned 3 where 0 was expected: aslr_x: no"):
        ext.conclude(REFUSED, OK, _outs(), "aslr_x: no", "aslr_x")
    with pytest.raises(AssertionError, match="aslr_x returned 0 where 3 was expected"):
        ext.conclude(OK, REFUSED, _outs(), "", "aslr_x")
    with pytest.raises(AssertionError, match="returned 5 where 3 was expected"):
        ext.conclude(5, REFUSED, _outs(), "another refusal")


def test_the_upload():
    assert ext.dev("cpu", None) is None and ext.dev("cpu", None, (1, 0)) is None
    v = np.arange(6, dtype=np.float32).reshape(2, 3)
    t = ext.dev("cpu", v, (1, 0))
    assert t.dtype == torch.float64 and tuple(t.shape) == (3, 2) and t.is_contiguous()
    np.testing.assert_array_equal(t.numpy(), v.T)
    np.testing.assert_array_equal(ext.dev("cpu", v).numpy(), v)
