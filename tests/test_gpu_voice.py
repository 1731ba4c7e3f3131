"""GPU parity for the voice-recorder symbol path (wavehip.voice): DiscriminatorDemodulator (decoders/p25.py:1105-1345)
and VoiceRecorder.process_iq's discriminator (trunking/system.py:708-717) vs the reference goldens of
tools/gen_golden_voice.py -- dibits and counts bit-exact, float32 state bit-exact, float64 state to 1e-12, type flags
equal -- plus the bank's own contracts (64-channel bank == 64 single demodulators, masking, growth, resets)."""

import ctypes

import numpy as np
import pytest

import signals as S
from conftest import peak_rel_err

pytestmark = pytest.mark.gpu

VARS = ("symbol_clock", "symbol_spread", "dc_estimate", "fine_freq_correction", "coarse_freq_correction", "input_gain")


def standalone_case(g, ci):
    fs = int(g[f"k{ci}_rate"])
    raw = g[f"k{ci}_audio"]
    x = raw.astype(np.float32) / 32768.0 if raw.dtype == np.int16 else raw   # process_discriminator's int16 rule
    lens = [int(v) for v in g[f"k{ci}_lens"]]
    resets = {int(v) for v in g[f"k{ci}_resets"] if v >= 0}
    return fs, x, lens, resets


def check_state(st, vals, flags, hist, hidx, count, where):
    for k, name in enumerate(VARS):
        assert st[name + "_is_f32"] == bool(flags[k]), (where, name, st[name + "_is_f32"])
        if flags[k]:
            assert np.float32(st[name]) == np.float32(vals[k]) and st[name] == float(np.float32(st[name])), \
                (where, name, st[name], vals[k])
        else:
            assert abs(st[name] - vals[k]) <= 1e-12 * max(abs(vals[k]), 1e-300), (where, name, st[name], vals[k])
    assert st["history"].tobytes() == np.asarray(hist, dtype=np.float32).tobytes(), where
    assert st["history_idx"] == hidx and st["symbol_count"] == count, where


def test_discriminator_demodulator_goldens(golden):
    import wavehip

    g = golden("voice")
    for ci in range(int(g["n_cases"])):
        fs, x, lens, resets = standalone_case(g, ci)
        d = wavehip.DiscriminatorDemodulator(sample_rate=fs)
        assert np.array_equal(d._baseband_taps, g["bb_taps" if fs == 48000 else "bb_taps_50k"])
        dib, pos = [], 0
        for k, ln in enumerate(lens):
            if k in resets:
                d.reset()
            o = d.demodulate(x[pos:pos + ln])
            pos += ln
            assert o.dtype == np.uint8 and len(o) == int(g[f"k{ci}_counts"][k]), (ci, k, len(o))
            dib.append(o)
            # state against the reference run whose low-pass is accumulated in float64 (what the device computes): numpy's
            # own float32 convolve sums through the CPU's BLAS sdot, so only that run is bit-reproducible; the dibits and
            # counts are the np.convolve run's, unchanged under that difference by the golden's case selection
            check_state(d.state(), g[f"k{ci}_vals_f64lpf"][k], g[f"k{ci}_flags"][k], g[f"k{ci}_hist_f64lpf"][k],
                        int(g[f"k{ci}_hidx"][k]), int(g[f"k{ci}_symcount"][k]), (str(g[f"k{ci}_name"]), k))
        assert np.array_equal(np.concatenate(dib), g[f"k{ci}_dibits"]), str(g[f"k{ci}_name"])
    assert wavehip.DiscriminatorDemodulator().demodulate(np.zeros(0, np.float32)).size == 0


def recorder_input(g):
    fs, chunk, seed = int(g["fs"]), int(g["chunk"]), int(g["seed"])
    n = chunk * len(g["plan_kind"])
    x = S.c4fm_iq(n, fs, seed, snr_db=25.0, freq_offset_hz=412_500.0)[0]
    x = (x + np.roll(x, 7) * np.exp(-2j * np.pi * 1_237_500.0 * np.arange(x.size) / fs)).astype(np.complex64)
    assert S.sha256(x) == str(g["sha"])
    return fs, chunk, x


def _same_state(a, b):
    for k, v in a.items():
        if isinstance(v, np.ndarray):
            if v.tobytes() != b[k].tobytes():
                return False
        elif not (v == b[k] or (v != v and b[k] != b[k])):
            return False
    return True


def _disc_within_iq_error(disc, want, z, prev_mag, eps=1e-5):
    """disc audio vs the reference's: within eps of its peak, or -- for weak samples -- within what an IQ error of eps
    times the IQ peak (the DDC's own tolerance) moves the angle: eps * peak|z| * (1 / |z[i]| + 1 / |z[i-1]|) rad"""
    mag = np.abs(z).astype(np.float64)
    pk = float(mag.max()) if mag.size else 0.0
    prev = np.concatenate([[prev_mag if prev_mag is not None else (mag[0] if mag.size else 1.0)], mag[:-1]])
    with np.errstate(divide="ignore"):
        bound = eps * pk * (1.0 / mag + 1.0 / prev)
    err = np.abs(disc.astype(np.float64) - want.astype(np.float64))
    return bool(np.all(err <= np.maximum(eps * float(np.max(np.abs(want))), bound)))


def test_voice_recorder_bank_goldens(golden):
    import wavehip

    g = golden("voice_recorder")
    fs, chunk, x = recorder_input(g)
    offsets = [float(v) for v in g["offsets"]]
    reassign = {int(r[0]): (int(r[1]), float(r[2])) for r in g["reassign"]}
    R = len(offsets)
    bank = wavehip.VoiceRecorderBank(R, fs)
    for k, off in enumerate(offsets):
        bank.assign(k, off)
    # single-channel front-ends mirroring the bank's (bit-identical to it: test_n3_ddc_bank_voice_recorders): the
    # decimated IQ whose magnitude sets how far the complex64 IQ error can move each disc sample
    mirror = [wavehip.TrunkingDDC(fs, bank.ddc.stage1_factor, bank.ddc.stage2_factor) for _ in range(R)]
    prev_mag = [None] * R
    got = {k: dict(dib=[], disc=[], phase=[], phase_tol=[]) for k in range(R)}
    pos = {k: 0 for k in range(R)}
    for ci, kind in enumerate(g["plan_kind"]):
        part = x[ci * chunk:(ci + 1) * chunk]
        if kind == "zero":
            part = np.zeros(chunk, dtype=np.complex64)
        elif kind == "nan":
            part = part.copy()
            part[chunk // 3] = np.nan
        if ci in reassign:
            k, off = reassign[ci]
            bank.assign(k, off)
            offsets[k] = off
            mirror[k] = wavehip.TrunkingDDC(fs, bank.ddc.stage1_factor, bank.ddc.stage2_factor)
            prev_mag[k] = None
        active = [bool(v) for v in g["plan_active"][ci]]
        before = [bank.state(k) for k in range(R)]
        res = bank.process(part, active=active)
        for k in range(R):
            called = bool(g[f"r{k}_called"][ci])
            if called:
                assert res[k] is not None, (ci, k)
                got[k]["dib"].append(res[k][0])
                z = mirror[k].process(part, offsets[k])
                n = len(res[k][1])
                want = g[f"r{k}_disc"][pos[k]:pos[k] + n]
                pos[k] += n
                assert len(z) == n == len(want), (ci, k)
                peak_rel_err(res[k][1], want)                      # recorded in the margins table
                assert _disc_within_iq_error(res[k][1], want, z, prev_mag[k]), (ci, k)
                prev_mag[k] = float(np.abs(z[-1]))
                # the carried phase is the unwrapped angle of the call's last sample: same IQ error model
                got[k]["phase_tol"].append(1e-5 * float(np.abs(z).max()) / max(prev_mag[k], 1e-30))
                got[k]["disc"].append(res[k][1])
            else:   # idle, outside the band, or a NaN chunk: nothing ran and the state did not move
                assert res[k] is None, (ci, k)
                assert _same_state(before[k], bank.state(k)), (ci, k)
            if active[k]:
                got[k]["phase"].append(bank.state(k)["last_phase"])
                if not called:
                    got[k]["phase_tol"].append(got[k]["phase_tol"][-1] if got[k]["phase_tol"] else 0.0)
    for k in range(R):
        n_calls = int(np.sum(g[f"r{k}_called"]))
        assert len(got[k]["dib"]) == n_calls
        assert [len(v) for v in got[k]["dib"]] == [int(v) for v in g[f"r{k}_counts"]], k
        dib = np.concatenate(got[k]["dib"]) if got[k]["dib"] else np.zeros(0, np.uint8)
        assert np.array_equal(dib, g[f"r{k}_dibits"]), k
        if n_calls:
            assert [len(v) for v in got[k]["disc"]] == [int(v) for v in g[f"r{k}_disc_lens"]], k
        want = g[f"r{k}_phase"]
        assert len(got[k]["phase"]) == len(want), k
        for a, b, t in zip(got[k]["phase"], want, got[k]["phase_tol"]):
            assert abs(a - b) <= max(1e-9 * max(abs(b), 1.0), t), (k, a, b, t)
    assert bank.process(np.zeros(0, np.complex64)) == [None] * R


def _streams(n_ch, n, seed):
    """n_ch different disc-audio-like streams: C4FM-ish symbol levels, DC, noise, one muted channel"""
    rng = np.random.default_rng(seed)
    sym = rng.choice(np.array([-3, -1, 1, 3], dtype=np.float32), size=(n_ch, n // 10 + 2))
    x = np.repeat(sym, 10, axis=1)[:, :n] * rng.uniform(0.02, 0.2, size=(n_ch, 1)).astype(np.float32)
    x += rng.normal(0.0, 0.03, size=(n_ch, n)).astype(np.float32) + rng.uniform(-0.1, 0.1, size=(n_ch, 1)).astype(np.float32)
    if n_ch > 3:
        x[3] = 0.0
    return np.ascontiguousarray(x, dtype=np.float32)


def test_bank_of_64_equals_single_demodulators():
    import wavehip

    lens = [4800, 37, 7200, 99, 4800]
    x = _streams(64, sum(lens), 7)
    bank = wavehip.DiscriminatorBank(64)
    singles = [wavehip.DiscriminatorDemodulator() for _ in range(64)]
    pos = 0
    for ln in lens:
        res = bank.demodulate(x[:, pos:pos + ln])
        for c in range(64):
            o = singles[c].demodulate(x[c, pos:pos + ln])
            assert np.array_equal(res[c], o), (pos, c)
        pos += ln
    for c in range(64):
        assert _same_state(bank.state(c), singles[c].state()), c


def test_active_mask_and_nonfinite_rows():
    import wavehip

    x = _streams(4, 9600, 11)
    bank = wavehip.DiscriminatorBank(4)
    ref = [wavehip.DiscriminatorDemodulator() for _ in range(4)]
    first = bank.demodulate(x[:, :4800])
    for c in range(4):
        assert np.array_equal(first[c], ref[c].demodulate(x[c, :4800]))
    before = [bank.state(c) for c in range(4)]
    y = x[:, 4800:].copy()
    y[2, 100] = np.inf                       # channel 2: non-finite row -> dropped, state untouched
    res = bank.demodulate(y, active=[1, 0, 1, 1])
    assert res[1] is None and len(res[2]) == 0
    for c in (1, 2):
        assert _same_state(before[c], bank.state(c)), c
    for c in (0, 3):
        assert np.array_equal(res[c], ref[c].demodulate(x[c, 4800:])), c
        assert _same_state(bank.state(c), ref[c].state()), c


def test_long_call_grows_the_bank():
    import wavehip

    x = _streams(2, 20000, 5)
    small = wavehip.DiscriminatorBank(2, max_samples_per_call=1024)
    big = wavehip.DiscriminatorBank(2, max_samples_per_call=1 << 15)
    for sl in (slice(0, 800), slice(800, 15000), slice(15000, 20000)):
        a, b = small.demodulate(x[:, sl]), big.demodulate(x[:, sl])
        for c in range(2):
            assert np.array_equal(a[c], b[c])
    assert small.max_samples_per_call >= 14200
    for c in range(2):
        assert _same_state(small.state(c), big.state(c))


def test_resets():
    import wavehip

    x = _streams(1, 12000, 3)[0] * 3.0
    d = wavehip.DiscriminatorDemodulator()
    d.demodulate(x[:4800])
    g = d.state()
    assert g["input_gain_is_f32"] and g["input_gain"] != 1.0
    d.reset()                                        # DiscriminatorDemodulator.reset(): the gain survives
    s = d.state()
    assert s["input_gain"] == g["input_gain"] and s["input_gain_is_f32"]
    assert s["symbol_clock"] == 0.0 and not s["symbol_clock_is_f32"] and s["symbol_spread"] == 2.0
    assert s["symbol_count"] == 0 and s["history_idx"] == 0 and not s["history"].any()
    # full reset == a fresh object, on a bank channel next to a channel that keeps going
    bank = wavehip.DiscriminatorBank(2)
    bank.demodulate(np.stack([x[:4800], x[:4800]]))
    keep = bank.state(1)
    bank.reset(0, full=True)
    assert _same_state(bank.state(1), keep)
    fresh = wavehip.DiscriminatorDemodulator()
    a = bank.demodulate(np.stack([x[4800:], x[4800:]]))
    assert np.array_equal(a[0], fresh.demodulate(x[4800:]))
    assert _same_state(bank.state(0), fresh.state())


def test_run_argument_errors_with_a_live_handle():
    import torch
    import wavehip
    from wavehip import _lib

    bank = wavehip.DiscriminatorBank(2, max_samples_per_call=1024)
    lib, h = _lib.lib, bank._h
    x = torch.zeros((2, 2048), dtype=torch.float32, device="cuda")
    dib = torch.zeros((2, 2048), dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(2, dtype=torch.int32, device="cuda")
    st = _lib.stream_ptr(torch)
    before = [bank.state(c) for c in range(2)]
    bad = [
        lambda: lib.wh_disc_bank_run(h, x.data_ptr(), 2048, 2048, None, dib.data_ptr(), 2048, cnt.data_ptr(), st),  # n > max
        lambda: lib.wh_disc_bank_run(h, x.data_ptr(), 512, 256, None, dib.data_ptr(), 2048, cnt.data_ptr(), st),   # stride
        lambda: lib.wh_disc_bank_run(h, x.data_ptr(), 512, 2048, None, dib.data_ptr(), 256, cnt.data_ptr(), st),   # cap
        lambda: lib.wh_disc_bank_run(h, None, 512, 2048, None, dib.data_ptr(), 2048, cnt.data_ptr(), st),
        lambda: lib.wh_disc_bank_run(h, x.data_ptr(), 512, 2048, None, None, 2048, cnt.data_ptr(), st),
        lambda: lib.wh_disc_bank_run(h, x.data_ptr(), 512, 2048, None, dib.data_ptr(), 2048, None, st),
        lambda: lib.wh_disc_bank_run_iq(h, x.data_ptr(), 2048, 2048, None, None, dib.data_ptr(), 2048, cnt.data_ptr(), st),
        lambda: lib.wh_disc_bank_reset(h, 2, 0, st),
        lambda: lib.wh_disc_bank_reset(h, 0, 2, st),
        lambda: lib.wh_disc_bank_get_state(h, 2, (ctypes.c_double * 23)(), st),
        lambda: lib.wh_disc_bank_reserve(h, 0, st),
    ]
    for k, call in enumerate(bad):
        assert call() == -1, k
        assert b"wh_disc_bank" in lib.wh_last_error(), k
    for c in range(2):
        assert _same_state(before[c], bank.state(c))
