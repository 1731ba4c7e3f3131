"""Voice-recorder symbol path (wavehip.voice), host side only: the C ABI's argument checks, the exports and the host-side
filter designs against the reference's (tests/golden/voice.npz).  No GPU needed."""

import ctypes

import numpy as np


def _lib():
    from wavehip import _lib
    return _lib


def test_voice_symbols_exported():
    import wavehip
    from wavehip import voice

    lib = _lib().lib
    for name in ("wh_disc_bank_create", "wh_disc_bank_run", "wh_disc_bank_run_iq", "wh_disc_bank_reserve",
                 "wh_disc_bank_reset", "wh_disc_bank_get_state", "wh_disc_bank_destroy"):
        assert hasattr(lib, name), name
    for name in ("DiscriminatorBank", "DiscriminatorDemodulator", "VoiceRecorderBank"):
        assert getattr(wavehip, name) is getattr(voice, name)
        assert name in wavehip.__all__


def test_host_filter_designs_match_reference(golden):
    from wavehip import voice

    g = golden("voice")
    assert np.array_equal(voice.generate_mmse_taps(), g["mmse"])
    assert voice.generate_mmse_taps().dtype == np.float32
    assert np.array_equal(voice.design_baseband_filter(48000), g["bb_taps"])
    assert np.array_equal(voice.design_baseband_filter(50000), g["bb_taps_50k"])


def test_create_argument_errors_leave_handle_untouched():
    L = _lib()
    lib = L.lib
    bb = np.ones(65, dtype=np.float32)
    mm = np.ones(129 * 8, dtype=np.float32)
    even = np.ones(64, dtype=np.float32)
    h = ctypes.c_void_p()
    bad = [
        (None, 4, 48000.0, 4800.0, L.dptr(bb, "f32"), 65, L.dptr(mm, "f32"), 4800),    # null out
        ("h", 0, 48000.0, 4800.0, L.dptr(bb, "f32"), 65, L.dptr(mm, "f32"), 4800),     # no channels
        ("h", 1025, 48000.0, 4800.0, L.dptr(bb, "f32"), 65, L.dptr(mm, "f32"), 4800),  # too many channels
        ("h", 4, 0.0, 4800.0, L.dptr(bb, "f32"), 65, L.dptr(mm, "f32"), 4800),         # sample rate
        ("h", 4, float("nan"), 4800.0, L.dptr(bb, "f32"), 65, L.dptr(mm, "f32"), 4800),
        ("h", 4, 48000.0, 0.0, L.dptr(bb, "f32"), 65, L.dptr(mm, "f32"), 4800),        # symbol rate
        ("h", 4, 48000.0, 48000.0, L.dptr(bb, "f32"), 65, L.dptr(mm, "f32"), 4800),    # symbol rate >= sample rate
        ("h", 4, 48000.0, 4800.0, None, 65, L.dptr(mm, "f32"), 4800),                  # null taps
        ("h", 4, 48000.0, 4800.0, L.dptr(even, "f32"), 64, L.dptr(mm, "f32"), 4800),   # even filter length
        ("h", 4, 48000.0, 4800.0, L.dptr(bb, "f32"), 0, L.dptr(mm, "f32"), 4800),
        ("h", 4, 48000.0, 4800.0, L.dptr(bb, "f32"), 65, None, 4800),                  # null MMSE table
        ("h", 4, 48000.0, 4800.0, L.dptr(bb, "f32"), 65, L.dptr(mm, "f32"), 0),        # no samples per call
    ]
    for args in bad:
        h.value = None
        out = ctypes.byref(h) if args[0] else None
        assert lib.wh_disc_bank_create(out, *args[1:]) == -1, args
        assert b"wh_disc_bank_create" in lib.wh_last_error()
        assert not h.value, args


def test_run_argument_errors_and_null_handles():
    lib = _lib().lib
    # null handle: an argument error on every entry point, never a crash
    assert lib.wh_disc_bank_run(None, None, 16, 16, None, None, 16, None, None) == -1
    assert b"wh_disc_bank_run" in lib.wh_last_error()
    assert lib.wh_disc_bank_run_iq(None, None, 16, 16, None, None, None, 16, None, None) == -1
    assert b"wh_disc_bank_run_iq" in lib.wh_last_error()
    assert lib.wh_disc_bank_reserve(None, 4096, None) == -1
    assert b"wh_disc_bank_reserve" in lib.wh_last_error()
    assert lib.wh_disc_bank_reset(None, -1, 0, None) == -1
    assert b"wh_disc_bank_reset" in lib.wh_last_error()
    out = (ctypes.c_double * 23)()
    assert lib.wh_disc_bank_get_state(None, 0, out, None) == -1
    assert b"wh_disc_bank_get_state" in lib.wh_last_error()
    lib.wh_disc_bank_destroy(None)    # a no-op
