"""The integer identities behind the depth kernel's high-byte requant (k_cnn.hip: requant4_i8_hi), as a numpy model of the instructions the
kernel issues, against the plain definition clamp(x >> s, 0, 255) - 128; and the host's choice of the form (fasthevc_amd/weights.py:
requant_modes, the restatement of build_weight_image's).  Exact: every comparison is array_equal."""
import numpy as np
import pytest

from fasthevc_amd import weights

INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1


def _sat16(v):
    return np.clip(v, -32768, 32767)


def _cvt_pk_i16_i32(x):
    """v_cvt_pk_i16_i32 on one half: int32 -> int16 with saturation"""
    assert x.dtype == np.int32
    return _sat16(x.astype(np.int64)).astype(np.int16)


def _pk_add_i16_clamp(p):
    """v_pk_add_i16 p, p clamp on one half: saturating doubling"""
    assert p.dtype == np.int16
    return _sat16(2 * p.astype(np.int64)).astype(np.int16)


def _high_byte(p):
    """what v_perm_b32 with selector 0x07050301 gathers: byte 1 of each 16-bit half, read as the signed byte the kernel stores"""
    assert p.dtype == np.int16
    return (p.view(np.uint16) >> 8).astype(np.uint8).view(np.int8)


def high_byte_requant(x, shift):
    """the kernel's form on the accumulators x (int64, before the fold): the host adds - (128 << shift) to the bias, the MFMA delivers
    int32, then 8 - shift saturating doublings between the pack and the gather"""
    y = x - (128 << shift)
    assert y.min() >= INT32_MIN and y.max() <= INT32_MAX, "the folded accumulator must fit int32: the host's check"
    p = _cvt_pk_i16_i32(y.astype(np.int32))
    for _ in range(8 - shift):
        p = _pk_add_i16_clamp(p)
    return _high_byte(p)


def plain_requant(x, shift):
    return (np.clip(x >> shift, 0, 255) - 128).astype(np.int8)


def _inputs(shift):
    fold = 128 << shift
    top = (1 << 31) - 1 - fold   # the largest |accumulator| the host's check admits: bound + (128 << shift) < 2^31
    edge = np.array([1 << 23, -(1 << 23), (1 << 23) - 1, 1 - (1 << 23), 1 << 30, -(1 << 30), top, -top, top - 1, 1 - top,
                     fold - 1, fold, fold + 1, 255 << shift, (256 << shift) - 1, 256 << shift, -1, 0, 1], np.int64)
    return np.concatenate([np.arange(-(1 << 21), 1 << 21, dtype=np.int64), edge])


@pytest.mark.parametrize("shift", [8, 7])
def test_high_byte_form_equals_shift_clamp_minus_128(shift):
    x = _inputs(shift)
    got, exp = high_byte_requant(x, shift), plain_requant(x, shift)
    assert np.array_equal(got, exp), x[np.nonzero(got != exp)[0][:8]]
    assert exp.min() == -128 and exp.max() == 127 and len(np.unique(exp)) == 256   # both clamps and every byte in between


def test_the_doubling_is_needed_at_shift_7_and_wrong_at_shift_8():
    """the two forms are not interchangeable: the model tells them apart (so the sweep above is not vacuous)"""
    x = np.arange(0, 1 << 16, dtype=np.int64)
    for shift, doublings in ((7, 0), (8, 1)):
        p = _cvt_pk_i16_i32((x - (128 << shift)).astype(np.int32))
        for _ in range(doublings):
            p = _pk_add_i16_clamp(p)
        assert not np.array_equal(_high_byte(p), plain_requant(x, shift))


def test_the_chooser_takes_the_high_byte_forms_only_as_a_pair_and_only_where_the_fold_fits():
    m = weights.requant_modes
    small = 1 << 20
    assert m(7, 8, small, small) == (3, 3, (-(128 << 7), -(128 << 8)))
    # where mode 2 used to step aside (bound >= 2^23) the high-byte form still holds
    assert m(7, 8, small, 1 << 24) == (3, 3, (-(128 << 7), -(128 << 8)))
    # the other shifts, and the knobs that keep today's forms and biases
    assert m(8, 7, small, small) == (2, 1, (0, 0))
    assert m(6, 8, small, small) == (1, 2, (0, 0))
    assert m(7, 8, small, small, requant="short") == (1, 2, (0, 0))
    assert m(7, 8, small, 1 << 24, requant="short") == (1, 0, (0, 0))
    assert m(7, 8, small, small, requant="general") == (0, 0, (0, 0))
    assert m(7, 8, small, small, trio=True) == (1, 2, (0, 0))
    # a bound whose fold would wrap int32 is refused, for either layer, and BOTH layers fall back to the forms and biases of before
    last3, last2 = (1 << 31) - (128 << 8) - 1, (1 << 31) - (128 << 7) - 1
    assert m(7, 8, small, last3) == (3, 3, (-(128 << 7), -(128 << 8)))
    assert m(7, 8, small, last3 + 1) == (1, 0, (0, 0))
    assert m(7, 8, last2, small) == (3, 3, (-(128 << 7), -(128 << 8)))
    assert m(7, 8, last2 + 1, small) == (1, 2, (0, 0))
    # ... and at the last admitted bound the folded accumulator is exactly representable and requantises right
    for shift, last in ((8, last3), (7, last2)):
        x = np.array([last, -last], np.int64)
        assert np.array_equal(high_byte_requant(x, shift), plain_requant(x, shift))
        with pytest.raises(AssertionError):   # (the check is one short of int32's asymmetric end: -(last + 1) folds to -2^31 exactly)
            high_byte_requant(np.array([-(last + 2)], np.int64), shift)


def test_the_blobs_of_the_gpu_tests_take_the_forms_they_are_meant_to():
    def modes(w, **kw):
        return weights.requant_modes(int(w["shift"][1]), int(w["shift"][2]), weights.requant_bound(w["w2"], w["b2"]),
                                     weights.requant_bound(w["w3"], w["b3"]), **kw)[:2]
    w = weights.random_weights(11)
    for shifts, exp in (((6, 7, 8), (3, 3)), ((6, 8, 7), (2, 1)), ((6, 6, 8), (1, 2))):
        w["shift"] = np.array(shifts, np.int32)
        assert modes(w) == exp, shifts
    w["shift"] = np.array((6, 7, 8), np.int32)
    assert modes(w, requant="short") == (1, 2)
    assert modes(weights.requant_limit_weights("high")) == (3, 3) and modes(weights.requant_limit_weights("high"), requant="short") == (1, 0)
    for over in (False, True):
        assert modes(weights.requant_limit_weights(3, over)) == (3, 3)                       # conv2 at shift 7, conv3 at the 2^23 limit
        assert modes(weights.requant_limit_weights(3, over), requant="short") == (1, 0 if over else 2)
        assert modes(weights.requant_limit_weights(2, over)) == (0 if over else 2, 2)        # conv2 at shift 8: no high-byte pair
