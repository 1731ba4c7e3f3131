"""P25 channel front (wavehip.p25front), host side only: exports, the C ABI's argument checks, the Python argument
errors, and the rate / up-down / tap plan against decimate_iq_for_p25's formulas (capture.py:203-295) and
scipy.signal.resample_poly itself.  No GPU needed."""

import ctypes
from math import gcd

import numpy as np
import pytest
from scipy import signal

ALL_RATES = (2_400_000, 1_920_000, 480_000, 96_000, 200_000, 64_000, 250_000, 1_000_000, 2_048_000, 6_000_000,
             8_000_000, 48_000, 19_200, 12_000)


def _lib():
    from wavehip import _lib
    return _lib


def reference_plan(fs):
    """decimate_iq_for_p25's branches, restated: (kind, output rate, subsample step, up, down)."""
    if fs <= 48000:
        return "pass", fs, 1, 1, 1
    g = gcd(fs, 48000)
    up, down = 48000 // g, fs // g
    if down > 50:
        d = fs // 48000
        return "subsample", fs // d, d, up, down
    return "resample", fs * up // down, down, up, down


def test_p25front_exported():
    import wavehip
    from wavehip import p25front

    lib = _lib().lib
    for name in ("wh_p25front_create", "wh_p25front_set_offsets", "wh_p25front_out_len", "wh_p25front_run",
                 "wh_p25front_destroy"):
        assert hasattr(lib, name), name
    for name in ("P25ChannelBank", "P25ChannelFront", "decimate_iq_for_p25"):
        assert getattr(wavehip, name) is getattr(p25front, name)
        assert name in wavehip.__all__


def test_plan_matches_reference_formulas():
    from wavehip import p25front as P

    for fs in ALL_RATES:
        kind, rate, step, up, down = reference_plan(fs)
        p = P.p25_plan(fs)
        assert (p["kind"], p["rate"], p["step"]) == (kind, rate, step), fs
        if kind != "pass":
            assert (p["up"], p["down"]) == (up, down), fs
    # the rates the issue lists
    assert P.p25_plan(2_400_000)["down"] == 50 and P.p25_plan(1_920_000)["down"] == 40
    assert P.p25_plan(480_000)["down"] == 10 and P.p25_plan(96_000)["down"] == 2
    assert [P.p25_plan(f)["step"] for f in (250_000, 1_000_000, 2_048_000, 6_000_000, 8_000_000)] == [5, 20, 42, 125, 166]
    assert [P.p25_plan(f)["rate"] for f in (6_000_000, 8_000_000, 1_000_000)] == [48_000, 48_192, 50_000]


def test_out_len_matches_resample_poly_and_slicing():
    from wavehip import p25front as P

    for fs in ALL_RATES:
        kind, _, step, up, down = reference_plan(fs)
        for n in (1, 7, 333, 4099, max(8192, fs // 20) + 7):
            if kind == "resample":
                want = len(signal.resample_poly(np.zeros(n, dtype=np.float32), up, down))
            else:
                want = len(np.zeros(n)[::step])
            assert P.out_len(n, fs) == want, (fs, n)


def test_taps_are_resample_polys():
    """resample_poly's filter, read back from its own output: an impulse at sample k with up == 1 gives y[m] = h[m down
    + d0 - k]; compared in full for 1/2 and against firwin's design for every resample rate."""
    from wavehip import p25front as P

    for fs in ALL_RATES:
        kind, _, _, up, down = reference_plan(fs)
        if kind != "resample":
            continue
        h = P.resample_poly_taps(up, down)
        mx = max(up, down)
        assert h.dtype == np.float32 and len(h) == 20 * mx + 1
        want = signal.firwin(20 * mx + 1, 1.0 / mx, window=("kaiser", 5.0)).astype(np.float32)
        want *= np.float32(up)
        assert np.array_equal(h, want), fs


def emulate_kernel(x, up, down, h):
    """p25f_resample_kernel's index plan and float32 order, restated in numpy: y[m] = sum over i (descending) of
    x[q0 - i] * h[i up + t - pre_pad], P = (n_pre_remove + m) down, q0 = P // up, t = P % up."""
    L = len(h)
    half_len = (L - 1) // 2
    pre_pad = down - half_len % down
    n_pre_remove = (half_len + pre_pad) // down
    nu = len(x) * up
    m = nu // down + bool(nu % down)
    y = np.zeros(m, dtype=np.float32)
    for k in range(m):
        P = (n_pre_remove + k) * down
        q0, t = P // up, P % up
        i = np.arange((L - 1 + pre_pad - t) // up, -1, -1)
        j = i * up + t - pre_pad
        s = q0 - i
        ok = (j >= 0) & (j < L) & (s >= 0) & (s < len(x))
        prod = (x[s[ok]] * h[j[ok]]).astype(np.float32)
        y[k] = np.add.accumulate(np.r_[np.float32(0), prod], dtype=np.float32)[-1] if prod.size else 0
    return y


@pytest.mark.parametrize("fs,n", [(2_400_000, 2207), (96_000, 301), (200_000, 777), (64_000, 95), (480_000, 150)])
def test_kernel_index_plan_is_resample_poly_bit_for_bit(fs, n):
    from wavehip import p25front as P

    p = P.p25_plan(fs)
    h = P.resample_poly_taps(p["up"], p["down"])
    x = np.random.default_rng(fs + n).standard_normal(n).astype(np.float32)
    want = signal.resample_poly(x, p["up"], p["down"])
    assert want.dtype == np.float32
    assert np.array_equal(emulate_kernel(x, p["up"], p["down"], h), want)


def test_c_abi_argument_errors():
    L = _lib()
    lib = L.lib
    h = ctypes.c_void_p()
    taps = np.ones(1001, dtype=np.float32)
    tp = L.dptr(taps, "f32")
    assert lib.wh_p25front_create(None, 1, 6_000_000, None, 0) == -1
    assert lib.wh_p25front_create(ctypes.byref(h), 0, 6_000_000, None, 0) == -1 and not h.value
    assert lib.wh_p25front_create(ctypes.byref(h), 1, 0, None, 0) == -1 and not h.value
    assert lib.wh_p25front_create(ctypes.byref(h), 1, 2_400_000, None, 1001) == -1 and not h.value   # needs taps
    assert lib.wh_p25front_create(ctypes.byref(h), 1, 2_400_000, tp, 1000) == -1 and not h.value     # wrong count
    assert "1001" in lib.wh_last_error().decode()
    assert lib.wh_p25front_out_len(None, 100) == 0
    assert lib.wh_p25front_run(None, None, 10, None, None, 10, None) == -1
    assert lib.wh_p25front_set_offsets(None, None) == -1
    # a subsampling front owns no device memory: created and checked without a GPU
    assert lib.wh_p25front_create(ctypes.byref(h), 2, 6_000_000, None, 0) == 0 and h.value
    try:
        assert lib.wh_p25front_out_len(h, 250) == 2 and lib.wh_p25front_out_len(h, 251) == 3
        assert lib.wh_p25front_set_offsets(h, None) == -1
        bad = np.array([0.0, np.nan])
        assert lib.wh_p25front_set_offsets(h, L.dptr(bad, "f64")) == -1
        ok = np.array([12_500.5, -1e6])
        assert lib.wh_p25front_set_offsets(h, L.dptr(ok, "f64")) == 0
        fake = ctypes.c_void_p(4096)      # never dereferenced: every check below fails before any HIP call
        assert lib.wh_p25front_run(h, None, 1000, None, fake, 100, None) == -1
        assert lib.wh_p25front_run(h, fake, 1000, None, None, 100, None) == -1
        assert lib.wh_p25front_run(h, fake, 1000, None, fake, 7, None) == -1       # out_len(1000) == 8
        assert "out_stride" in lib.wh_last_error().decode()
        assert lib.wh_p25front_run(h, fake, (1 << 24) + 1, None, fake, 1 << 20, None) == -1
        assert lib.wh_p25front_run(h, None, 0, None, None, 0, None) == 0             # empty chunk: nothing to do
    finally:
        lib.wh_p25front_destroy(h)


def test_python_argument_errors():
    from wavehip import P25ChannelBank, P25ChannelFront
    from wavehip import p25front as P

    with pytest.raises(ValueError, match="Phase 2"):
        P25ChannelBank(2, 2_400_000, modulation="phase2")
    with pytest.raises(ValueError, match="upsample"):
        P25ChannelBank(2, 16_000)                      # pass-through at 16 kHz < 19 200 Hz
    with pytest.raises(ValueError):
        P25ChannelBank(0, 2_400_000)
    with pytest.raises(ValueError):
        P25ChannelFront(0, 2_400_000)
    with pytest.raises(ValueError):
        P25ChannelFront(1, 2_400_000, max_samples_per_call=(1 << 24) + 1)
    with pytest.raises(ValueError):
        P.p25_plan(0)
