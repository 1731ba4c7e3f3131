"""GPU parity tests: the HIP path (through the C ABI / host shims) against the golden
vectors captured from the reference and against the CPU oracle on seeded inputs.

Tolerances: bit-exact for int16 pack/unpack; TOL = 1e-5 peak-relative for float outputs
(north_star)."""

import numpy as np
import pytest

import signals as S
from conftest import db_close, peak_rel_err, record_margin

pytestmark = pytest.mark.gpu
TOL = 1e-5


@pytest.fixture(scope="module")
def wh():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    import wavehip

    return wavehip


@pytest.fixture(scope="module")
def O():
    from oracle import ref_np

    return ref_np


def test_a1_int16_bit_exact(wh, golden, O):
    g = golden("a1_int16")
    i16 = g["i16"]
    inter = np.stack([i16, i16[::-1]], axis=1).reshape(-1)
    z = wh.unpack_iq16(inter)
    assert np.array_equal(z.real, g["unpack_f32"]) and np.array_equal(z.imag, g["unpack_f32"][::-1])
    assert np.array_equal(np.frombuffer(wh.pack_iq16(g["pack_in"]), dtype=np.int16), g["pack_out"])
    assert np.array_equal(np.frombuffer(wh.pack_pcm16(g["pcm_in"]), dtype=np.int16), g["pcm_out"])
    # round trip on a large random buffer against the oracle
    x = S.noise_c64(1 << 20, 5, amp=0.4)
    p = np.frombuffer(wh.pack_iq16(x), dtype=np.int16)
    assert np.array_equal(p, O.pack_iq16(x))
    assert np.array_equal(wh.unpack_iq16(p), O.unpack_iq16(p))
    assert wh.pack_iq16(np.empty(0, np.complex64)) == b""


def _nco(wh, iq, off, fs):
    import torch
    from wavehip import _lib

    d = torch.from_numpy(iq).cuda()
    o = torch.empty_like(d)
    _lib.check(_lib.lib.wh_nco_mix(d.data_ptr(), o.data_ptr(), d.numel(), int(off), int(fs), _lib.stream_ptr(torch)))
    return o.cpu().numpy()


def test_a2_nco(wh, golden, O):
    g = golden("a2_nco")
    for ci in range(int(g["n_cases"])):
        n, off, fs, seed = (int(v) for v in g[f"c{ci}_args"])
        iq = S.noise_c64(n, seed)
        idx = g[f"c{ci}_idx"]
        y = _nco(wh, iq, off, fs)
        assert peak_rel_err(y[idx], g[f"c{ci}_y"]) <= TOL
        assert peak_rel_err(y, O.freq_shift(iq, float(off), fs)) <= TOL
    # the phasor itself (unit input) against the reference table: catches a float64-phase NCO
    n, off, fs, _ = (int(v) for v in g["c0_args"])
    tab = _nco(wh, np.ones(n, np.complex64), off, fs)
    assert np.max(np.abs(tab[g["c0_idx"]] - g["c0_tab"])) <= 1e-6


def test_a3_discriminator(wh, golden, O):
    import torch
    from wavehip import _lib

    g = golden("a3_quad")
    for iq, fs, y in ((g["iq"], int(g["fs"]), g["y"]), (g["iq2"], int(g["fs2"]), g["y2"])):
        d = torch.from_numpy(iq).cuda()
        o = torch.empty(d.numel(), dtype=torch.float32, device="cuda")
        _lib.check(_lib.lib.wh_fm_discriminate(d.data_ptr(), o.data_ptr(), d.numel(), fs, _lib.stream_ptr(torch)))
        assert peak_rel_err(o.cpu().numpy(), y) <= TOL


def test_a6_resample(wh, golden, O):
    import ctypes as C

    import torch
    from wavehip import _lib
    from wavehip.channel_ops import resample_design

    g = golden("a6_resample")
    for ci in range(int(g["n_cases"])):
        fi, fo, n, seed = (int(v) for v in g[f"c{ci}_args"])
        x = (np.random.default_rng(seed).standard_normal(n) * 0.3).astype(np.float32)
        h, up, down, d0 = resample_design(fi, fo)
        n_out = len(g[f"c{ci}_y"])
        r = C.c_void_p()
        _lib.check(_lib.lib.wh_resampler_create(C.byref(r), _lib.dptr(h, "f64"), len(h), up, down, d0))
        xb = np.stack([x, -0.5 * x])                       # batch of 2 rows
        d = torch.from_numpy(xb).cuda()
        o = torch.empty((2, n_out), dtype=torch.float32, device="cuda")
        _lib.check(_lib.lib.wh_resampler_run(r, d.data_ptr(), n, 2, o.data_ptr(), n_out, _lib.stream_ptr(torch)))
        y = o.cpu().numpy()
        _lib.lib.wh_resampler_destroy(r)
        assert peak_rel_err(y[0], g[f"c{ci}_y"]) <= TOL
        assert peak_rel_err(y[1], -0.5 * g[f"c{ci}_y"]) <= TOL


def _nbfm_cfg(wh, off):
    return wh.ChannelConfig(id="g", mode="nbfm", offset_hz=float(off), enable_deemphasis=False,
                            enable_mpx_filter=False)


def test_chain_nbfm_golden_int16_bank(wh, golden, O):
    """Config 2 shape: one int16 stream, 32 NBFM channels, against reference goldens (3 channels)
    and the oracle (all 32)."""
    g = golden("chain_analog")
    fs, n, seed0 = (int(v) for v in g["nbfm_args"])
    offs = S.nbfm_bank_offsets()
    bank = wh.ChannelBank(fs, n, [_nbfm_cfg(wh, o) for o in offs], input_format="int16")
    for chunk in range(2):
        i16 = S.pack_iq16_np(S.nbfm_bank_c64(n, fs, seed=seed0 + chunk, start=chunk * n))
        res = bank.process(i16)
        for k in g["nbfm_k"]:
            audio, met = res[int(k)]
            assert peak_rel_err(audio, g[f"nbfm{chunk}_k{k}_audio"]) <= TOL
            assert db_close([met["rssi_db"], met["signal_power_db"]], g[f"nbfm{chunk}_k{k}_met"])
        if chunk == 0:
            z = O.unpack_iq16(i16)
            for k in range(32):
                a_ref, m_ref = O.process_channel_nbfm(z, fs, offs[k])
                assert peak_rel_err(res[k][0], a_ref) <= TOL, k
                assert db_close(res[k][1]["rssi_db"], m_ref["rssi_db"])


def test_chain_nbfm_single_channel_dropin(wh, golden):
    g = golden("chain_analog")
    fs, n, seed0 = (int(v) for v in g["nbfm_args"])
    offs = S.nbfm_bank_offsets()
    i16 = S.pack_iq16_np(S.nbfm_bank_c64(n, fs, seed=seed0, start=0))
    z = wh.unpack_iq16(i16)
    audio, met = wh.process_channel_dsp_stateless(z, fs, _nbfm_cfg(wh, offs[13]))
    assert audio.dtype == np.float32 and audio.shape == (2400,)
    assert peak_rel_err(audio, g["nbfm0_k13_audio"]) <= TOL
    # error conventions (capture.py:321-325)
    assert wh.process_channel_dsp_stateless(np.empty(0, np.complex64), fs, _nbfm_cfg(wh, 0)) == (None, {})
    bad = z.copy()
    bad[100] = np.nan
    assert wh.process_channel_dsp_stateless(bad, fs, _nbfm_cfg(wh, offs[13])) == (None, {})
    with pytest.raises(NotImplementedError):
        wh.process_channel_dsp_stateless(z, fs, wh.ChannelConfig(mode="cw"))        # not a reference mode either


def test_chain_nbfm_multichunk_matches_single(wh):
    """n_chunks in one launch == chunk-by-chunk (stateless per chunk, capture.py:298)."""
    import torch

    fs, n = 2400000, 120000
    offs = S.nbfm_bank_offsets(8)
    bank = wh.ChannelBank(fs, n, [_nbfm_cfg(wh, o) for o in offs], input_format="int16")
    i16 = np.concatenate([S.pack_iq16_np(S.nbfm_bank_c64(n, fs, seed=40 + c, n_ch=8, start=c * n)) for c in range(3)])
    a3, m3 = bank.process_device(torch.from_numpy(i16).cuda(), 3)
    a3 = a3.cpu().numpy()
    for c in range(3):
        a1, _ = bank.process_device(torch.from_numpy(i16[2 * n * c: 2 * n * (c + 1)].copy()).cuda(), 1)
        assert np.array_equal(a1.cpu().numpy()[0], a3[c])


def test_n1_signal_metrics(wh, golden, O):
    """Channel.update_signal_metrics for all 32 channels in one pass: RSSI + exact 10/90-percentile SNR."""
    g = golden("chain_analog")
    fs, n, seed0 = (int(v) for v in g["nbfm_args"])
    iq = S.nbfm_bank_c64(n, fs, seed=seed0, start=0)
    offs = S.nbfm_bank_offsets()
    res = wh.update_signal_metrics(iq, fs, offs)
    for row, k in zip(g["sigmet"], (0, 13, 31)):
        assert db_close(res[k]["rssi_db"], row[0]) and db_close(res[k]["snr_db"], row[1])
    for k in (5, 20):
        rssi, snr = O.update_signal_metrics(iq, fs, offs[k])
        assert db_close(res[k]["rssi_db"], rssi) and db_close(res[k]["snr_db"], snr)
    # int16 input and a zero offset (no mix)
    i16 = S.pack_iq16_np(iq)
    r2 = wh.update_signal_metrics(i16, fs, [0.0, offs[3]], input_format="int16")
    z = O.unpack_iq16(i16)
    for got, off in zip(r2, (0.0, offs[3])):
        rssi, snr = O.update_signal_metrics(z, fs, off)
        assert db_close(got["rssi_db"], rssi) and db_close(got["snr_db"], snr)
    # one ranking of |iq| for all channels (no mix: |freq_shift(iq)| = |iq| up to float32 rounding) against the
    # reference goldens of three channels, and through the dispatcher (one upload, snr_db on every channel)
    sh = wh.update_signal_metrics(iq, fs, offs, shared_magnitudes=True)
    for row, k in zip(g["sigmet"], (0, 13, 31)):
        assert db_close(sh[k]["rssi_db"], row[0]) and db_close(sh[k]["snr_db"], row[1])
    cfgs = [wh.ChannelConfig(mode="nbfm", offset_hz=offs[k], enable_deemphasis=False) for k in (0, 13, 31)]
    out = wh.ChannelDispatcher(fs).process(iq, cfgs, snr=True)
    for (audio, m), row in zip(out, g["sigmet"]):
        assert audio is not None and db_close(m["rssi_db"], row[0]) and db_close(m["snr_db"], row[1])


def test_chain_wbfm(wh, golden):
    g = golden("chain_analog")
    for ci in range(2):
        fs, n, seed, off = (int(v) for v in g[f"wbfm{ci}_args"])
        iq = S.fm_tone_c64(n, fs, seed=seed, carrier_hz=float(off))
        cfg = wh.ChannelConfig(id="w", mode="wbfm", offset_hz=float(off))
        audio, met = wh.process_channel_dsp_stateless(iq, fs, cfg)
        assert peak_rel_err(audio, g[f"wbfm{ci}_audio"]) <= TOL
        assert db_close([met["rssi_db"], met["signal_power_db"]], g[f"wbfm{ci}_met"])


def test_chain_am_ssb_filtered_fm(wh, golden, O):
    """Dispatcher modes am / ssb (AGC, Butterworth, BFO) and NBFM with every optional IIR stage,
    against the reference goldens, plus the oracle on a second seed."""
    from test_oracle_golden import analog_cases

    g = golden("chain_analog")
    C = wh.ChannelConfig
    cfgs = {
        "am48": C(mode="am", offset_hz=4800.0, enable_agc=True),
        "am48to24": C(mode="am", offset_hz=4800.0, enable_agc=True, audio_rate=24000),
        "am48noagc": C(mode="am", offset_hz=4800.0, enable_agc=False),
        "am96nohp": C(mode="am", offset_hz=9600.0, enable_agc=True, enable_am_highpass=False),
        "ssb32usb": C(mode="ssb", offset_hz=3200.0, enable_agc=True, ssb_mode="usb"),
        "ssb32lsb": C(mode="ssb", offset_hz=3200.0, enable_agc=True, ssb_mode="lsb"),
        "nbfmf96": C(mode="nbfm", offset_hz=12000.0, enable_deemphasis=True, enable_fm_highpass=True,
                     fm_highpass_hz=300, enable_fm_lowpass=True, fm_lowpass_hz=3000, notch_frequencies=[1000.0]),
    }
    for tag, mk, fs, off, demod, kw in analog_cases():
        iq = mk()
        audio, met = wh.process_channel_dsp_stateless(iq, fs, cfgs[tag])
        assert audio is not None and audio.shape == g[f"{tag}_audio"].shape, tag
        assert peak_rel_err(audio, g[f"{tag}_audio"]) <= TOL, tag
        assert db_close([met["rssi_db"], met["signal_power_db"]], g[f"{tag}_met"]), tag
    # a bank of 3 AM channels on one chunk vs the oracle
    fs, n = 48000, 4800
    iq = (S.am_tone_c64(n, fs, 61, carrier_hz=3000.0) + S.am_tone_c64(n, fs, 62, carrier_hz=-7000.0, audio_hz=500.0)
          + S.am_tone_c64(n, fs, 63, carrier_hz=12000.0, audio_hz=1200.0)).astype(np.complex64)
    offs = [3000.0, -7000.0, 12000.0]
    res = wh.ChannelBank(fs, n, [C(mode="am", offset_hz=o, enable_agc=True) for o in offs]).process(iq)
    for k, o in enumerate(offs):
        a_ref, _ = O.process_channel(iq, fs, o, O.am_demod)
        assert peak_rel_err(res[k][0], a_ref) <= TOL, k


def test_a7_pfb_golden(wh, golden):
    g = golden("a7_pfb")
    for ci in range(int(g["n_cases"])):
        fs, bw, M, seed, n1, n2 = (int(v) for v in g[f"c{ci}_args"])
        x = S.noise_c64(n1 + n2, seed)
        ch = wh.PolyphaseChannelizer(fs, bw)
        assert ch.channel_count == M and S.sha256(ch.arms) == str(g[f"c{ci}_arms_sha"])
        r1 = ch.process(x[:n1])
        r2 = ch.process(x[n1:])
        assert r1.shape == g[f"c{ci}_r1"].shape and r2.shape == g[f"c{ci}_r2"].shape
        assert peak_rel_err(r1, g[f"c{ci}_r1"]) <= TOL
        assert peak_rel_err(r2, g[f"c{ci}_r2"]) <= TOL
        assert np.array_equal(ch.arm_history, g[f"c{ci}_hist"])
        assert peak_rel_err(ch.extract_channel(r1, 5), g[f"c{ci}_ex5"]) <= TOL
        assert len(list(r1)) == r1.shape[0] and r1[0].shape == (M,)      # list-like view
        ch.reset()
        assert not ch.arm_history.any()
    ch = wh.PolyphaseChannelizer(1_000_000, 25000)
    assert len(ch.process(S.noise_c64(39, 1))) == 0


@pytest.mark.parametrize("n", [1024 * 9 + 512 * 3, 1024 * 300 + 77, 512 * 4099 + 1024])
def test_a7_pfb_fast_path_vs_oracle(wh, O, n):
    """M=1024 sizes that exercise the fused kernel (hops >= 8), its ragged tail and the
    carried history across two calls."""
    x = S.noise_c64(n + 5000, 77)
    ch = wh.PolyphaseChannelizer(10_000_000, 9765)
    ref = O.PolyphaseChannelizer(10_000_000, 9765)
    for part in (x[:n], x[n:]):
        a, b = ch.process(part), ref.process(part)
        assert a.shape == b.shape
        assert peak_rel_err(a, b) <= TOL
    assert np.array_equal(ch.arm_history, ref.arm_history)


def test_a7_pfb_properties_large(wh):
    """Size-independent properties at a size the oracle would not finish quickly:
    linearity and the response to a single complex tone (energy lands in one channel)."""
    import torch

    n = 1 << 24
    ch = wh.PolyphaseChannelizer(10_000_000, 9765)
    g = torch.Generator(device="cuda").manual_seed(3)
    a = torch.randn(n, 2, device="cuda", generator=g).mul_(0.5)
    b = torch.randn(n, 2, device="cuda", generator=g).mul_(0.5)
    xa, xb = torch.view_as_complex(a), torch.view_as_complex(b)
    ya = ch.process_device(xa).clone(); ch.reset()
    yb = ch.process_device(xb).clone(); ch.reset()
    ys = ch.process_device(xa * 0.5 + xb * 2.0); ch.reset()
    err = (ys - (ya * 0.5 + yb * 2.0)).abs().max().item() / ys.abs().max().item()
    assert err <= 1e-5
    # tone at the centre of channel 37: x[n] = exp(2 pi i 37 n / 1024)
    k = 37
    t = torch.arange(n, device="cuda", dtype=torch.float64)
    ph = 2 * np.pi * ((t * k) % 1024) / 1024
    tone = torch.complex(torch.cos(ph), torch.sin(ph)).to(torch.complex64)
    yt = ch.process_device(tone)
    p = (yt[16:].abs() ** 2).mean(0)
    assert int(p.argmax()) == k
    assert p[k].item() > 0.75 * p.sum().item()   # the reference's structure leaks into k+-1 (no per-hop shift)


def test_a7_pfb_int16_input(wh):
    """int16 IQ input (unpack fused into the loads) == unpack first, bit for bit; both paths + history."""
    import torch

    x = S.noise_c64(1024 * 200 + 333, 12, amp=0.25)
    i16 = S.pack_iq16_np(x)
    xq = wh.unpack_iq16(i16)
    for fs, bw in ((10_000_000, 9765), (1_000_000, 25000)):
        a, b = wh.PolyphaseChannelizer(fs, bw), wh.PolyphaseChannelizer(fs, bw)
        for lo, hi in ((0, 150000), (150000, len(xq))):
            ya = a.process_device(torch.from_numpy(i16[2 * lo:2 * hi].copy()).cuda())
            yb = b.process_device(torch.from_numpy(xq[lo:hi].copy()).cuda())
            assert torch.equal(ya, yb)
        assert np.array_equal(a.arm_history, b.arm_history)


@pytest.mark.parametrize("engine", ["fused", "stockham"])
def test_a8_spectrum(wh, golden, engine):
    """engine "fused" = the library's choice (the shaped kernel at the goldens' sizes 512 .. 4096); "stockham" = the
    kernel serving the other power-of-two sizes, forced."""
    g = golden("a8_spectrum")
    for ci in range(int(g["n_cases"])):
        N, fs, seed = (int(v) for v in g[f"c{ci}_args"])
        iq = S.fm_tone_c64(N + 100, fs, seed=seed, deviation=20000.0, carrier_hz=123456.0, noise_amp=0.01)
        be = wh.HipFFTBackend(N, engine=engine)
        r = be.execute(iq, fs)
        assert be.name == "hip" and r.power_db.dtype == np.float32 and r.freqs.dtype == np.float32
        ref = g[f"c{ci}_power"]
        lin, lin_ref = 10.0 ** (r.power_db / 20.0), 10.0 ** (ref / 20.0)
        assert peak_rel_err(lin, lin_ref) <= TOL                     # magnitude, peak-relative
        strong = ref > ref.max() - 60.0
        assert np.max(np.abs(r.power_db[strong] - ref[strong])) <= 0.01   # dB on bins within 60 dB
        assert int(np.argmax(r.power_db)) == int(np.argmax(ref))
        assert np.array_equal(r.freqs, g[f"c{ci}_freqs"]) and r.bin_hz == float(g[f"c{ci}_bin"])
    r = wh.HipFFTBackend(1024).execute(S.noise_c64(100, 1), 2400000)     # short input -> zeros
    assert not r.power_db.any() and not r.freqs.any()
    # non power of two size goes through the direct DFT
    be = wh.HipFFTBackend(1000)
    iq = S.fm_tone_c64(1000, 1_000_000, seed=9, deviation=5000.0, carrier_hz=50_000.0)
    from oracle import ref_np as O
    p, f, b = O.spectrum(iq, 1_000_000, 1000)
    r = be.execute(iq, 1_000_000)
    assert peak_rel_err(10.0 ** (r.power_db / 20.0), 10.0 ** (p / 20.0)) <= TOL


@pytest.mark.parametrize("N", [256, 512, 1024, 2048, 4096])
def test_a8_spectrum_shaped_kernel_batches(wh, O, N):
    """The shaped spectrum kernel (pfb_mid.hip spectrum_mid_kernel) on batches: frame counts that do not fill the last
    workgroup, overlapping frames (frame_stride < N) and strides > N; every frame equals the oracle to 1e-5 (linear
    magnitude, peak-relative) and, bit for bit, the same frame run alone; a silent frame gives -200 dB; enough
    frames for several rounds per workgroup (the prefetch path)."""
    import torch

    with pytest.raises(RuntimeError):
        wh.HipFFTBackend(8192, engine="shaped")
    be = wh.HipFFTBackend(N, engine="shaped")
    x = S.fm_tone_c64(N * 40 + 777, 2_400_000, seed=3000 + N, deviation=30000.0, carrier_hz=-234567.0, noise_amp=0.02)
    x[N * 20: N * 22] = 0
    xd = torch.from_numpy(x).cuda()
    worst = 0.0
    for frames, stride in ((1, N), (3, N), (37, N), (13, N // 2 + 3), (9, 3 * N + 5)):
        out = be.execute_device(xd, frames, stride).cpu().numpy()
        for f in range(frames):
            seg = x[f * stride: f * stride + N]
            ref = O.spectrum(seg, 2_400_000, N)[0]
            if not seg.any():
                assert np.all(np.abs(out[f] + 200.0) <= 1e-4)       # 20 log10(0 + 1e-10)
                continue
            err = peak_rel_err(10.0 ** (out[f] / 20.0), 10.0 ** (ref / 20.0))
            worst = max(worst, err)
            assert err <= TOL, (N, frames, stride, f)
            strong = ref > ref.max() - 60.0
            assert np.max(np.abs(out[f][strong] - ref[strong])) <= 0.01
        if frames > 5:
            one = be.execute_device(xd[5 * stride: 5 * stride + N].contiguous(), 1)
            assert np.array_equal(out[5], one[0].cpu().numpy())
    print(f"spectrum shaped N={N}: worst peak-relative error {worst:.2e}")
    # many rounds per workgroup: 3 x (CUs x resident workgroups) frame groups, compared with the Stockham kernel
    frames = 20000 if N <= 1024 else 6000
    g = torch.Generator(device="cuda").manual_seed(N)
    big = torch.view_as_complex(torch.randn(frames * N, 2, device="cuda", generator=g) * 0.3)
    a = be.execute_device(big, frames)
    b = wh.HipFFTBackend(N, engine="stockham").execute_device(big, frames)
    lin = lambda p: 10.0 ** (p.double() / 20.0)
    assert ((lin(a) - lin(b)).abs().amax(1) / lin(b).amax(1)).max().item() <= TOL
    pick = torch.tensor([0, 1, frames // 2, frames - 2, frames - 1], device="cuda")
    for f in pick.tolist():
        assert torch.equal(a[f], be.execute_device(big[f * N: (f + 1) * N].contiguous(), 1)[0])


def test_a8_spectrum_rocfft_engine_and_batch(wh, golden, O):
    """The rocFFT engine (HIP window/epilogue kernels around a rocFFT batched C2C) gives the reference
    spectrum too, and batched frames equal frame-by-frame execution for both engines."""
    import time

    import torch

    g = golden("a8_spectrum")
    for ci in range(int(g["n_cases"])):
        N, fs, seed = (int(v) for v in g[f"c{ci}_args"])
        iq = S.fm_tone_c64(N + 100, fs, seed=seed, deviation=20000.0, carrier_hz=123456.0, noise_amp=0.01)
        r = wh.HipFFTBackend(N, engine="rocfft").execute(iq, fs)
        ref = g[f"c{ci}_power"]
        assert peak_rel_err(10.0 ** (r.power_db / 20.0), 10.0 ** (ref / 20.0)) <= TOL
    N, frames = 2048, 4096
    x = torch.view_as_complex(torch.randn(frames * N, 2, device="cuda") * 0.3)
    outs = {}
    for eng in ("fused", "stockham", "rocfft"):
        be = wh.HipFFTBackend(N, engine=eng)
        outs[eng] = be.execute_device(x, frames)
        one = be.execute_device(x[5 * N: 6 * N].contiguous(), 1)
        assert torch.equal(outs[eng][5], one[0])
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(10):
            be.execute_device(x, frames)
        torch.cuda.synchronize()
        print(f"spectrum {eng}: {frames * N * 10 / (time.perf_counter() - t0) / 1e9:.2f} GS/s")
    lin = lambda p: 10.0 ** (p.double() / 20.0)
    assert ((lin(outs["fused"]) - lin(outs["rocfft"])).abs().max() / lin(outs["rocfft"]).max()).item() <= TOL


def test_a13_channel_stats(wh, O):
    import torch

    x = S.noise_c64(1024 * 64, 91)
    ch = wh.PolyphaseChannelizer(10_000_000, 9765)
    y = ch.process_device(torch.from_numpy(x).cuda())
    st = ch.channel_stats_device(y).cpu().numpy()
    ref = O.pfb_channel_stats(y.cpu().numpy())
    # the statistic's definition: p in float32 (count, min, max exact), sums of short float32 blocks in float64 (<= 2e-6)
    assert np.array_equal(st[:, 2:], ref[:, 2:])
    assert np.allclose(st[:, :2], ref[:, :2], rtol=2e-6, atol=0)
    record_margin(float(np.max(np.abs(st[:, :2] - ref[:, :2]) / ref[:, :2])), tol=2e-6)
    st2 = ch.channel_stats_device(y, torch.from_numpy(st.copy()).cuda(), accumulate=True).cpu().numpy()
    assert np.allclose(st2[:, :2], 2 * st[:, :2], rtol=1e-15) and np.array_equal(st2[:, 2], 2 * ref[:, 2])
    assert np.array_equal(st2[:, 3:], ref[:, 3:])
    # accumulate into an EMPTY row (count 0, e.g. a zero-initialised buffer) == overwrite: its zeros are no observations
    st3 = ch.channel_stats_device(y, torch.zeros_like(torch.from_numpy(st)).cuda(), accumulate=True).cpu().numpy()
    assert np.array_equal(st3, st)


def test_a4_a5_trunking_ddc(wh, golden, O):
    """Phase-continuous NCO + two-stage decimator: reference golden (ragged calls, offset change,
    index wrap) and a second seed against the oracle."""
    g = golden("trunk")
    fs, d1, d2, seed = (int(v) for v in g["ddc_args"])
    lens, offs = [int(v) for v in g["ddc_lens"]], [float(v) for v in g["ddc_offs"]]
    x = S.c4fm_iq(sum(lens), fs, seed, snr_db=25.0, freq_offset_hz=312500.0)[0]
    ddc = wh.TrunkingDDC(fs, d1, d2)
    assert (ddc.stage1_factor, ddc.stage2_factor) == wh.decimation_plan(fs) == (d1, d2)
    pos, outs = 0, []
    for n, off in zip(lens, offs):
        outs.append(ddc.process(x[pos:pos + n], off))
        pos += n
    assert [len(o) for o in outs] == [int(v) for v in g["ddc_counts"]]
    assert peak_rel_err(np.concatenate(outs), g["ddc_out"]) <= TOL
    # reset() + no-mix path vs the oracle, single stage
    x2 = S.noise_c64(300000, 9)
    a, b = wh.TrunkingDDC(1_000_000, 20, 1), O.TrunkingDDC(1_000_000, 20, 1)
    for part in (x2[:100000], x2[100000:100007], x2[100007:]):
        assert peak_rel_err(a.process(part, 0.0), b.process(part, 0.0)) <= TOL
    a.reset(); b.reset()
    assert peak_rel_err(a.process(x2[:5000], 12345.0), b.process(x2[:5000], 12345.0)) <= TOL


def test_a13_scanner_measure(wh, golden, O):
    from test_oracle_golden import _scan_buffer

    g = golden("trunk")
    fs, n, seed = (int(v) for v in g["scan_args"])
    w = _scan_buffer(n, fs, seed)
    res = wh.ScannerMeasure(fs).measure(w, [float(v) for v in g["scan_offsets"]])
    got = np.array([[m["power_db"], m["peak_power_db"], m["noise_floor_db"], m["snr_db"], m["sample_count"]]
                    for m in res])
    assert db_close(got[:, :4], g["scan_meas"][:, :4])
    assert np.array_equal(got[:, 4], g["scan_meas"][:, 4])
    order = np.argsort(-got[:, 3])
    assert order[0] == 0 and order[1] == 1            # the two carriers rank first by SNR
    # sync-pattern check on a buffer with a real C4FM carrier: flags == reference, correlation ~ oracle
    from test_oracle_golden import _scan_buffer2
    w2 = _scan_buffer2(n, fs)
    offs = [float(v) for v in g["scan_offsets"]]
    res2 = wh.ScannerMeasure(fs).measure(w2, offs)
    ref2 = O.scanner_measure(w2, fs, offs, sync_check=True)
    got2 = np.array([[m["power_db"], m["peak_power_db"], m["noise_floor_db"], m["snr_db"]] for m in res2])
    assert db_close(got2, g["scan2_meas"][:, :4])
    assert [float(m["sync_detected"]) for m in res2] == list(g["scan2_meas"][:, 4])
    for a, b in zip(res2, ref2):
        assert abs(a["sync_correlation"] - b["sync_correlation"]) <= 1e-6


def test_n2_soft_sync_detector(wh, golden, O):
    """P25P1SoftSyncDetector.process_batch on ragged calls (incl. n < 24, n == 0) vs reference scores;
    tolerance 1e-5 of peak (24-term f32 dot product, summation order differs from np.correlate)."""
    g = golden("framer")
    det = wh.P25P1SoftSyncDetector()
    assert np.array_equal(det.SYNC_PATTERN_SYMBOLS, g["pattern"])
    pos, outs = 0, []
    for n in g["lens"]:
        outs.append(det.process_batch(g["soft"][pos:pos + int(n)]))
        pos += int(n)
    got = np.concatenate(outs)
    assert got.dtype == np.float32 and got.shape == g["scores"].shape
    assert peak_rel_err(got, g["scores"]) <= 1e-5
    # the sync positions score 24 * 9 = 216 nominal: same argmax set as the reference
    assert np.array_equal(np.nonzero(got > 150)[0], np.nonzero(g["scores"] > 150)[0])
    det.reset()
    single = np.array([det.process(float(v)) for v in g["soft"][:64]], dtype=np.float32)
    assert peak_rel_err(single, g["single"]) <= 1e-5


def test_n2_soft_sync_bank_matches_per_channel(wh, O):
    import torch
    rng = np.random.default_rng(1710)
    C, n = 37, 5000
    soft = rng.uniform(-4, 4, (C, 2 * n)).astype(np.float32)
    bank = wh.SoftSyncBank(C)
    a = bank.process_device(torch.from_numpy(soft[:, :n].copy()).cuda()).cpu().numpy()
    b = bank.process_device(torch.from_numpy(soft[:, n:].copy()).cuda()).cpu().numpy()
    for c in (0, 17, C - 1):
        ref = O.SoftSyncDetector()
        want = np.concatenate([ref.process_batch(soft[c, :n]), ref.process_batch(soft[c, n:])])
        assert peak_rel_err(np.concatenate([a[c], b[c]]), want) <= 1e-5


def test_n4_pack_f32(wh, golden):
    g = golden("framer")
    assert wh.pack_f32(g["f32_in"]) == g["f32_out"].tobytes()
    assert wh.pack_f32(np.array([], dtype=np.float32)) == b""


def test_chain_raw_and_digital_modes(wh, golden):
    """capture.py:415-430 branches of the operator: "raw" (shifted IQ interleaved, validated like audio) and
    the digital voice modes (metrics only)."""
    g = golden("chain_rawdig")
    fs, n, seed = (int(v) for v in g["args"])
    iq = S.nbfm_bank_c64(n, fs, seed=seed)
    for ci, off in enumerate(g["offs"]):
        audio, met = wh.process_channel_dsp_stateless(iq, fs, wh.ChannelConfig(mode="raw", offset_hz=float(off)))
        assert audio.dtype == np.float32 and audio.shape == (2 * n,)
        assert peak_rel_err(audio, g[f"raw{ci}_audio"]) <= TOL
        assert db_close([met["rssi_db"], met["signal_power_db"]], g[f"raw{ci}_met"])
        for mode in ("p25", "dmr", "nxdn", "dstar", "ysf"):
            audio, met = wh.process_channel_dsp_stateless(iq, fs, wh.ChannelConfig(mode=mode, offset_hz=float(off)))
            assert audio is None
            assert db_close([met["rssi_db"], met["signal_power_db"]], g[f"dig{ci}_met"])
    audio, met = wh.process_channel_dsp_stateless((iq * 40).astype(np.complex64), fs, wh.ChannelConfig(mode="raw"))
    assert audio is None and "signal_power_db" not in met and db_close(met["rssi_db"], float(g["loud_rssi"]))
    bad = iq.copy()
    bad[5] = np.nan
    assert wh.process_channel_dsp_stateless(bad, fs, wh.ChannelConfig(mode="raw")) == (None, {})


def test_chain_sam(wh, golden):
    """"sam" mode (dsp/sam.py:132-269 through capture.py:386-399): float64 carrier-recovery PLL per chunk,
    sideband selection, then the AM chain; single-channel operator and a 3-channel bank."""
    from test_oracle_golden import sam_cases
    g = golden("chain_sam")
    for tag, fs, iq, off, kw in sam_cases(g):
        cfg = wh.ChannelConfig(mode="sam", offset_hz=off, **kw)
        audio, met = wh.process_channel_dsp_stateless(iq, fs, cfg)
        assert audio is not None and audio.shape == g[f"{tag}_audio"].shape, tag
        assert peak_rel_err(audio, g[f"{tag}_audio"]) <= TOL, tag
        assert db_close([met["rssi_db"], met["signal_power_db"]], g[f"{tag}_met"]), tag
    tag, fs, iq, off, kw = next(sam_cases(g))
    cfgs = [wh.ChannelConfig(mode="sam", offset_hz=o, **kw) for o in (off - 50.0, off, off + 50.0)]
    res = wh.ChannelBank(fs, iq.shape[0], cfgs).process(iq)
    assert peak_rel_err(res[1][0], g[f"{tag}_audio"]) <= TOL
    assert res[0][0] is not None and res[2][0] is not None


def test_chain_am_ssb_sam_at_capture_rates(wh, golden):
    """AM / SSB / SAM where the live loop runs them: 250 kS/s and 2.4 MS/s chunks (`chain_caprate`, from the reference).
    The reference's order-5 ba-form Butterworths are ill-conditioned at these rates (a +-1-ulp input perturbation moves
    the AM audio by 4e-4 at 250 kS/s and by 0.4 at 2.4 MS/s; the SSB band-pass overflows), so what the goldens pin is what
    the live loop acts on (capture.py:323-325, 2593-2595): the OUTCOME CLASS -- audio, or None because
    validate_audio_samples fails (validation.py:41-52) -- and the metrics; the audio itself wherever the measured
    sensitivity `sens` is below 1e-3, to max(1e-5, 4 * sens); signal_power_db to max(2e-4 dB, 4 x the shift the same
    perturbation gives the reference's own value)."""
    import ast
    g = golden("chain_caprate")
    n_audio = 0
    for tag in [str(t) for t in g["tags"]]:
        fs, n, seed, car, off = g[f"{tag}_args"]
        iq = S.am_tone_c64(int(n), int(fs), seed=int(seed), carrier_hz=float(car), depth=0.7)
        assert S.sha256(iq) == str(g[f"{tag}_sha"])
        kw = ast.literal_eval(str(g[f"{tag}_kw"]))
        cfg = wh.ChannelConfig(mode=str(g[f"{tag}_mode"]), offset_hz=float(off), **kw)
        audio, met = wh.process_channel_dsp_stateless(iq, int(fs), cfg)
        want_audio = bool(int(g[f"{tag}_class"]))
        assert (audio is not None) == want_audio, (tag, "outcome class")
        ref_met, ref_pert = g[f"{tag}_met"], g[f"{tag}_met_pert"]
        assert db_close(met["rssi_db"], ref_met[0], label="rssi dB"), tag
        assert ("signal_power_db" in met) == want_audio, tag
        if not want_audio:
            continue
        sens = float(g[f"{tag}_sens"])
        sp_tol = max(2e-4, 4.0 * abs(float(ref_met[1] - ref_pert[1])))
        assert db_close(met["signal_power_db"], ref_met[1], tol=sp_tol,
                        label="signal power dB" if sp_tol == 2e-4 else "signal power dB (ill-conditioned)"), (tag, sp_tol)
        assert audio.shape == g[f"{tag}_audio"].shape, tag
        if sens < 1e-3:
            tol = max(TOL, 4.0 * sens)
            err = float(np.max(np.abs(audio - g[f"{tag}_audio"])) / np.max(np.abs(g[f"{tag}_audio"])))
            record_margin(err, tol, "audio" if tol == TOL else "audio at 4 x measured sensitivity")
            assert err <= tol, (tag, err, tol)
            n_audio += 1
    assert n_audio >= 5


def test_chain_fm_exact_zero_samples(wh, O, golden):
    """Muted input (a stretch of exact zeros, isolated zero samples): the reference's discriminator value of a sample whose
    conjugate product is exactly zero hangs on IEEE signed zeros -- numpy's complex product of a zero sample with the mixer
    phase gives (+-0, +-0) by the phase's quadrant, and np.angle = arctan2 maps (+-0, -0) to +-pi -- so a muted stretch
    comes out as 0 or +-pi x scale.  NBFM (the fused kernel: raw angles + mixer step, zero products evaluated by
    fm_single_zero) and WBFM (the unfused front) against the numpy oracle, which inherits numpy's semantics; int16 and
    complex64 input.  (Round 2 returned 0 for such samples: up to 0.2 of peak off on this input.)"""
    fs, n = 2_400_000, 120_000
    offs = S.nbfm_bank_offsets(32)[12:16]
    i16 = S.nbfm_zero_gap_i16(n, fs)
    z = i16.astype(np.float32) / 32768.0
    z = (z[0::2] + 1j * z[1::2]).astype(np.complex64)
    cfgs = [_nbfm_cfg(wh, o) for o in offs] + [_nbfm_cfg(wh, 0.0)]
    for fmt, src in (("int16", i16), ("cf32", z)):
        res = wh.ChannelBank(fs, n, cfgs, input_format=fmt).process(src)
        for k, cfg in enumerate(cfgs):
            a_ref, m_ref = O.process_channel_nbfm(z, fs, float(cfg.offset_hz))
            a, m = res[k]
            assert (a is None) == (a_ref is None), (fmt, k)
            if a is not None:
                assert peak_rel_err(a, a_ref) <= TOL, (fmt, k)
            assert db_close(m["rssi_db"], m_ref["rssi_db"]), (fmt, k)
    w = wh.ChannelConfig(mode="wbfm", offset_hz=200000.0)
    a, m = wh.process_channel_dsp_stateless(z, fs, w)
    a_ref, m_ref = O.process_channel_wbfm(z, fs, 200000.0)
    assert (a is None) == (a_ref is None)
    if a is not None:
        assert peak_rel_err(a, a_ref) <= TOL
    # ... and against the reference itself (tests/golden/chain_zero.npz: its discriminator of the muted stretch is 0 / 16)
    g = golden("chain_zero")
    assert S.sha256(i16) == str(g["sha_i16"])
    for k in range(3):
        au, me = wh.process_channel_dsp_stateless(z, fs, _nbfm_cfg(wh, float(g[f"nbfm{k}_off"][0])))
        assert peak_rel_err(au, g[f"nbfm{k}_audio"]) <= TOL and db_close([me["rssi_db"], me["signal_power_db"]], g[f"nbfm{k}_met"]), k
    assert peak_rel_err(a, g["wbfm_audio"]) <= TOL and db_close([m["rssi_db"], m["signal_power_db"]], g["wbfm_met"])


def test_chain_nbfm_extreme_offsets_vs_oracle(wh, O):
    """The fused NBFM front adds the mixer's float32 phase step to the raw discriminator angle and wraps: offsets next to
    +-fs / 2 (step ~ -+pi: every sample wraps), 1 Hz (step ~ 2.6e-6 rad), a non-integer offset (the reference rounds it,
    capture.py:173) and 0.4 Hz (rounds to 0 Hz but still takes the mixed branch: offset_hz != 0.0)."""
    fs, n = 2_400_000, 120_000
    i16 = S.pack_iq16_np(S.nbfm_bank_c64(n, fs, seed=88))
    z = i16.astype(np.float32) / 32768.0
    z = (z[0::2] + 1j * z[1::2]).astype(np.complex64)
    offs = [1_199_999.0, -1_199_990.0, 1.0, -37_500.6, 0.4, 600_000.0]
    cfgs = [_nbfm_cfg(wh, o) for o in offs]
    res = wh.ChannelBank(fs, n, cfgs, input_format="int16").process(i16)
    for k, o in enumerate(offs):
        a_ref, m_ref = O.process_channel_nbfm(z, fs, o)
        a, m = res[k]
        assert (a is None) == (a_ref is None), o
        if a is not None:
            assert peak_rel_err(a, a_ref) <= TOL, o
        assert db_close(m["rssi_db"], m_ref["rssi_db"]), o


def test_chain_spectral_noise_reduction(wh, golden):
    """enable_noise_reduction on the FM chains (dsp/filters.py:346-460): STFT / percentile floor / Wiener gain /
    ISTFT on the device; audio length follows the shortened row; < 1024-sample chunks pass through.
    Tolerance: 1e-5 of peak everywhere except the first / last 8 audio samples, where 1e-3 is allowed: the
    reference divides the overlap-added frames by the summed squared Hann window, which falls to ~1e-10 at the
    two row edges, so the float32 FFT's own rounding (pocketfft there, an LDS Stockham FFT here) is amplified
    by 1/w(t) for the few samples next to each edge (measured: interior <= 2e-7, edges <= 5e-5)."""
    from test_oracle_golden import nr_cases
    g = golden("chain_nr")
    for tag, mode, fs, iq, off, db in nr_cases(g):
        if mode == "nbfm":
            cfg = _nbfm_cfg(wh, off)
        else:
            cfg = wh.ChannelConfig(mode="wbfm", offset_hz=off)
        cfg.enable_noise_reduction = True
        cfg.noise_reduction_db = db
        audio, met = wh.process_channel_dsp_stateless(iq, fs, cfg)
        assert audio is not None and audio.shape == g[f"{tag}_audio"].shape, (tag, None if audio is None else audio.shape)
        ref = g[f"{tag}_audio"]
        err = np.abs(audio - ref) / np.max(np.abs(ref))
        record_margin(err[8:-8].max(), TOL, 'interior'); record_margin(err.max(), 1e-3, '8 samples next to a row edge')
        assert err[8:-8].max() <= TOL and err.max() <= 1e-3, (tag, err[8:-8].max(), err.max())
        assert db_close([met["rssi_db"], met["signal_power_db"]], g[f"{tag}_met"]), tag
    # a call of more than 65535 rows (chunks x channels) is refused
    import torch
    cfg = _nbfm_cfg(wh, 0.0)
    cfg.enable_noise_reduction = True
    bank = wh.ChannelBank(2_400_000, 1024, [cfg] * 256)
    x = torch.zeros(257 * 1024, dtype=torch.complex64, device="cuda")
    with pytest.raises(RuntimeError, match="65535 rows"):
        bank.process_device(x, 257)


def test_n1_squelch_in_bank(wh):
    """capture.py:2918-2921 fused into the bank: a channel whose rssi_db is below its squelch_db returns zeros
    (metrics untouched); channels without a threshold or above it are unchanged."""
    fs, n = 2400000, 120000
    offs = S.nbfm_bank_offsets()
    iq = S.nbfm_bank_c64(n, fs, seed=580)
    base = [_nbfm_cfg(wh, offs[k]) for k in (3, 13, 20)]
    plain = wh.ChannelBank(fs, n, base).process(iq)
    sq = [_nbfm_cfg(wh, offs[k]) for k in (3, 13, 20)]
    sq[0].squelch_db = plain[0][1]["rssi_db"] + 1.0      # above the measured RSSI -> muted
    sq[1].squelch_db = plain[1][1]["rssi_db"] - 1.0      # below -> open
    got = wh.ChannelBank(fs, n, sq, apply_squelch=True).process(iq)
    assert np.all(got[0][0] == 0) and got[0][0].shape == plain[0][0].shape
    assert np.array_equal(got[1][0], plain[1][0]) and np.array_equal(got[2][0], plain[2][0])
    for a, b in zip(got, plain):
        assert a[1] == b[1]
    # without apply_squelch the thresholds are ignored (drop-in for the stateless operator)
    again = wh.ChannelBank(fs, n, sq).process(iq)
    assert np.array_equal(again[0][0], plain[0][0])


def test_n3_ddc_bank_voice_recorders(wh, golden, O):
    """TrunkingDDCBank: recorders sharing one 6 MS/s buffer (VoiceRecorder.process_iq, system.py:453-656) vs the
    reference goldens, incl. an idle chunk for one recorder, ragged calls and a 77-sample call; and every bank
    channel == the single-channel TrunkingDDC."""
    from test_oracle_golden import recorder_case
    g = golden("trunk_recorder")
    fs, x, lens = recorder_case(g)
    assert wh.recorder_decimation_plan(fs) == tuple(int(v) for v in g["factors"])
    offs = [float(v) for v in g["offsets"]] + [0.0, 1_000_000.0]
    bank = wh.TrunkingDDCBank(4, fs, plan="recorder")
    assert np.array_equal(bank.stage1_taps, g["t1"]) and np.array_equal(bank.stage2_taps, g["t2"])
    singles = [wh.TrunkingDDC(fs, bank.stage1_factor, bank.stage2_factor) for _ in offs]
    pos, outs = 0, [[] for _ in offs]
    for ci, ln in enumerate(lens):
        active = [1, 0 if ci == 1 else 1, 1, 1]
        res = bank.process(x[pos:pos + ln], offs, active)
        for k in range(4):
            if active[k]:
                outs[k].append(res[k])
                ref = singles[k].process(x[pos:pos + ln], offs[k])
                assert np.array_equal(res[k], ref), (ci, k)
            else:
                assert res[k] is None
        pos += ln
    for ri in (0, 1):
        assert [len(v) for v in outs[ri]] == [int(v) for v in g[f"r{ri}_counts"]]
        assert peak_rel_err(np.concatenate(outs[ri]), g[f"r{ri}_out"]) <= TOL
    # reset of one channel = a fresh front-end for that channel only
    bank.reset(2)
    res = bank.process(x[:5000], offs)
    fresh = wh.TrunkingDDC(fs, bank.stage1_factor, bank.stage2_factor).process(x[:5000], offs[2])
    assert np.array_equal(res[2], fresh)


def test_n4_channel_classifier(wh, golden):
    """ChannelClassifier drop-in: bin statistics accumulated on the device are BIT-IDENTICAL to the reference's
    Python-float BinStats (same float64 additions in the same order), classification equal; input as lists
    (the reference's call), numpy batches and GPU tensors straight from the spectrum backend."""
    import torch
    g = golden("classifier")
    p, freqs = S.classifier_frames()
    kinds = {"control": 0, "voice": 1, "variable": 2, "unknown": 3}
    for mode in ("list", "batch", "tensor"):
        cl = wh.ChannelClassifier(min_collection_seconds=0.0)
        if mode == "list":
            for f in range(p.shape[0]):
                cl.update(p[f].tolist(), freqs.tolist(), 851_000_000.0, 2_400_000.0)
        elif mode == "batch":
            for f in range(0, p.shape[0], 32):
                cl.update(p[f:f + 32], freqs, 851_000_000.0, 2_400_000.0)
        else:
            cl.update(torch.from_numpy(p).cuda(), freqs, 851_000_000.0, 2_400_000.0)
        assert cl.sample_count == int(g["sample_count"]) and cl.is_ready
        assert np.array_equal(cl.bin_stats(), g["stats"]), mode
        res = cl.classify(force=True)
        got = np.array([[c.freq_hz, c.power_db, c.std_dev_db, kinds[c.channel_type]] for c in res])
        assert np.array_equal(got, g["chans"]), mode
    # a parameter change clears the statistics (channel_classifier.py:104-110); reset() too
    cl.update(p[0], freqs, 852_000_000.0, 2_400_000.0)
    assert cl.sample_count == 1 and cl.get_status()["center_hz"] == 852_000_000.0
    cl.reset()
    assert cl.sample_count == 0 and cl.classify(force=True) == []
    # end to end: frames from the spectrum backend stay on the device
    be = wh.HipFFTBackend(512)
    iq = S.noise_c64(512 * 8, 1301)
    frames = be.execute_device(torch.from_numpy(iq).cuda(), n_frames=8)
    cl.update(frames.view(8, 512), freqs, 851_000_000.0, 2_400_000.0)
    assert cl.sample_count == 8 and cl.bin_stats().shape == (512, 5)


def test_n2_bch_decoder(wh, golden):
    """Exhaustive nearest-codeword BCH(63,16,23) on the device == the reference's bch_decode, bit for bit:
    360 golden words (0..14 errors, arbitrary words, tracked-NAC second pass) + the drop-in signature."""
    g = golden("nid")
    dec = wh.BCHDecoder()
    d, e = dec.decode_batch(g["words"], g["tracked"])
    assert np.array_equal(d, g["data"]) and np.array_equal(e, g["errors"])
    d0, e0 = dec.decode_batch(g["words"])                       # no tracked NAC: only first-pass results
    first = g["tracked"] == 0
    assert np.array_equal(d0[first], g["data"][first]) and np.array_equal(e0[first], g["errors"][first])
    w = int(g["words"][3])
    bits = np.array([(w >> (62 - i)) & 1 for i in range(63)], dtype=np.uint8)
    assert wh.bch_decode(bits, int(g["tracked"][3]) or None) == (int(g["data"][3]), int(g["errors"][3]))
    assert wh.bch_decode(np.zeros(63, dtype=np.uint8)) == (0, 0)            # reference tests/test_p25_bch.py:38-45
    for pos in range(63):                                                   # tests/test_reference_fec.py:212-231
        c = np.zeros(63, dtype=np.uint8)
        c[pos] = 1
        assert wh.bch_decode(c) == (0, 1)
    assert wh.bch_decode(np.zeros(10, dtype=np.uint8)) == (0, -1)
    # every codeword decodes to itself; 11 errors are corrected, 12 are not mis-corrected to the sent word
    from wavehip.fec import codeword_table
    t = codeword_table()
    rng = np.random.default_rng(1420)
    idx = rng.integers(0, 1 << 16, size=512)
    words = t[idx].copy()
    d, e = dec.decode_batch(words)
    assert np.array_equal(d, idx.astype(np.int32)) and not e.any()
    for k in range(512):
        for f in rng.choice(63, size=11, replace=False):
            words[k] ^= np.uint64(1) << np.uint64(int(f))
    d, e = dec.decode_batch(words)
    assert np.array_equal(d, idx.astype(np.int32)) and np.all(e == 11)


def test_n2_status_symbol_stripping(wh, golden, O):
    """wh_strip_status == P25Decoder._strip_status_symbols (decoders/p25.py:2796-2862) on the reference's own outputs
    (78 cases: lengths around the 36-dibit period, initial counters incl. 35, >= 36 and negative), bit for bit; batched
    rows with a row stride; a long row against the oracle."""
    import torch

    g = golden("status")
    for k in range(int(g["n_cases"])):
        r = wh.strip_status_symbols(g[f"c{k}_in"], int(g[f"c{k}_c0"]))
        assert r.dtype == np.uint8 and np.array_equal(r, g[f"c{k}_out"]), k
    assert wh.strip_status_symbols([], 21).size == 0
    rng = np.random.default_rng(2862)
    rows = rng.integers(0, 4, size=(7, 5000)).astype(np.uint8)
    wide = torch.from_numpy(np.concatenate([rows, rows[:, :13]], axis=1)).cuda()[:, :5000]      # row stride 5013
    for c0 in (21, 0, 35, 50):
        out = wh.strip_status_symbols_device(wide, c0).cpu().numpy()
        for c in range(7):
            assert np.array_equal(out[c], O.strip_status_symbols(rows[c], c0)), (c0, c)
    long = rng.integers(0, 4, size=1_000_003).astype(np.uint8)
    got = wh.strip_status_symbols(long, 21)
    keep = np.ones(long.size, dtype=bool)
    keep[14::36] = False                                   # first status symbol at 35 - 21
    assert np.array_equal(got, long[keep])


def test_n2_nid_front_end(wh, golden):
    """P25NIDFrontEnd == the NID events of the reference framer's process_batch (same ragged calls), and the events
    do not depend on how the stream is cut into calls."""
    g = golden("nid")
    dib, soft, heads = S.nid_stream()
    lens = [int(v) for v in g["lens"]]
    for cut in (lens, [97], [dib.size], [1000, 13]):
        fe = wh.P25NIDFrontEnd()
        ev, pos, k = [], 0, 0
        while pos < dib.size:
            ln = cut[k % len(cut)]
            k += 1
            ev += fe.process_batch(soft[pos:pos + ln], dib[pos:pos + ln])
            pos += ln
        assert np.array_equal(np.array(ev, dtype=np.int64), g["events"]), cut
    assert fe.nac_tracker.get_tracked_nac() == 0xC93
    fe.reset()
    assert fe.process_batch(soft[:300], dib[:300]) == [tuple(int(v) for v in r) for r in g["events"] if r[0] < 300]


def test_chain_wbfm_time_parallel_iir_equals_sequential(wh, golden):
    """The time-parallel form of the IIR rows (64 segments per wave and row; a segment's start states are the dot product
    of the warm-up samples before it with the chain's impulse-response states -- or, iir_form="warmup_recurrence", the
    recurrences run over those samples; used when the chain has no AGC and its impulse responses die out well inside
    the chunk) against the strictly sequential recurrence: same audio to ~1e-7 of peak (float32 stage rounding noise),
    all within the tolerance of the reference golden; and the warm-up length the host derives covers the slowest pole."""
    from wavehip.channel_ops import build_chain, iir_warmup_samples
    g = golden("chain_analog")
    fs, n, seed, off = (int(v) for v in g["wbfm1_args"])
    iq = S.fm_tone_c64(n, fs, seed=seed, carrier_hz=float(off))
    cfg = wh.ChannelConfig(mode="wbfm", offset_hz=float(off))
    stages = build_chain(cfg, fs)[2]
    warm = iir_warmup_samples(stages)
    assert 1898 < warm < 4000                       # butter(5, 15 kHz @ 2.4 MS/s): slowest pole radius 0.98794, 1e-10 after 1 898 samples
    par = wh.ChannelBank(fs, n, [cfg]).process(iq)[0][0]             # start states from the chain's impulse response
    rec = wh.ChannelBank(fs, n, [cfg], iir_form="warmup_recurrence").process(iq)[0][0]   # ... from the recurrences
    seq = wh.ChannelBank(fs, n, [cfg], iir_form="sequential").process(iq)[0][0]
    ref = g["wbfm1_audio"]
    assert peak_rel_err(par, ref) <= TOL and peak_rel_err(seq, ref) <= TOL and peak_rel_err(rec, ref) <= TOL
    assert peak_rel_err(par, seq) <= 1e-6 and peak_rel_err(rec, seq) <= 1e-6
    print(f"wbfm rows: impulse-response start states vs sequential {peak_rel_err(par, seq):.2e}, "
          f"warm-up recurrence vs sequential {peak_rel_err(rec, seq):.2e}")
    # several channels per bank (4 waves per row) and a ragged chunk length
    n2 = n - 4321
    cf3 = [wh.ChannelConfig(mode="wbfm", offset_hz=float(off) + k * 1e5) for k in range(20)]
    a = wh.ChannelBank(fs, n2, cf3).process(iq[:n2])
    b = wh.ChannelBank(fs, n2, cf3, iir_form="sequential").process(iq[:n2])
    assert max(peak_rel_err(a[k][0], b[k][0]) for k in range(20)) <= 1e-6
    # a chain whose poles are too slow for the chunk (or, in ba form at this rate, numerically on the unit circle)
    # stays sequential: warm-up 0 ("never") or longer than half the chunk
    hp = wh.ChannelConfig(mode="nbfm", offset_hz=0.0, enable_deemphasis=False, enable_fm_highpass=True, fm_highpass_hz=300)
    w = iir_warmup_samples(build_chain(hp, fs)[2])
    assert w == 0 or w > n // 2


def test_n1_channel_dispatcher_mixed_modes(wh, golden):
    """ChannelDispatcher = the DSP fan-out of Capture._process_channels_parallel (capture.py:2489-2597) in batched
    form: a mixed channel set (3 NBFM, 1 WBFM, raw, p25, NBFM with another filter set) on one chunk gives, per
    channel and in order, what process_channel_dsp_stateless gives -- and the NBFM rows match the reference goldens."""
    g = golden("chain_analog")
    fs, n, seed0 = (int(v) for v in g["nbfm_args"])
    offs = S.nbfm_bank_offsets()
    iq = wh.unpack_iq16(S.pack_iq16_np(S.nbfm_bank_c64(n, fs, seed=seed0, start=0)))
    cfgs = [_nbfm_cfg(wh, offs[0]), wh.ChannelConfig(mode="raw", offset_hz=offs[5]), _nbfm_cfg(wh, offs[13]),
            wh.ChannelConfig(mode="wbfm", offset_hz=0.0), wh.ChannelConfig(mode="p25", offset_hz=offs[7]),
            _nbfm_cfg(wh, offs[31]),
            wh.ChannelConfig(mode="nbfm", offset_hz=offs[20], enable_deemphasis=True, enable_fm_lowpass=True)]
    disp = wh.ChannelDispatcher(fs)
    res = disp.process(iq, cfgs)
    assert len(res) == len(cfgs) and len(disp._banks) == 3
    for k, i in ((0, 0), (13, 2), (31, 5)):
        assert peak_rel_err(res[i][0], g[f"nbfm0_k{k}_audio"]) <= TOL
        assert db_close([res[i][1]["rssi_db"], res[i][1]["signal_power_db"]], g[f"nbfm0_k{k}_met"])
    for i, c in enumerate(cfgs):
        a, m = wh.process_channel_dsp_stateless(iq, fs, c)
        if a is None:
            assert res[i][0] is None
        else:
            assert np.array_equal(res[i][0], a), i
        assert res[i][1] == m, i
    again = disp.process(iq, cfgs)                               # cached banks, same results
    assert len(disp._banks) == 3 and all(np.array_equal(a[0], b[0]) for a, b in zip(res, again) if a[0] is not None)
    bad = iq.copy()
    bad[3] = np.inf
    assert disp.process(bad, cfgs) == [(None, {})] * len(cfgs)
    assert disp.process(iq, []) == [] and disp.process(iq[:0], cfgs) == [(None, {})] * len(cfgs)


def test_chain_scan_form_equals_sequential(wh):
    """The exact scan form of the rows (zero-state pass, start states s' = M s + e, output pass; AGC envelopes
    likewise) against the strictly sequential kernel (WH_IIR_SEQ=1) at capture rate, for chains whose transition
    powers are well conditioned: AM envelope + AGC at capture rate, AM low-pass (+ AGC) at 96 kS/s.  Chains containing one of the
    reference's order-5 ba-form Butterworths are refused by the host check (|M| ~ 4e6 for the 100 Hz high-pass at
    48 kS/s; at 2.4 MS/s even the 5 kHz low-pass is clustered at z = 1) and stay sequential."""
    from wavehip.channel_ops import build_chain, iir_scan_safe
    C = wh.ChannelConfig
    cases = [
        (2_400_000, 120_000, C(mode="am", offset_hz=100e3, enable_agc=True, enable_am_highpass=False, enable_am_lowpass=False)),
        (96_000, 9_600, C(mode="am", offset_hz=9600.0, enable_agc=True, enable_am_highpass=False)),      # low-pass + AGC
        (96_000, 9_600, C(mode="am", offset_hz=9600.0, enable_agc=False, enable_am_highpass=False)),     # low-pass only
    ]
    assert not iir_scan_safe(build_chain(C(mode="am", enable_agc=True), 48000)[2], 75)
    assert not iir_scan_safe(build_chain(C(mode="am", enable_agc=True, enable_am_highpass=False), 2_400_000)[2], 1875)
    for k, (fs, n, cfg) in enumerate(cases):
        assert iir_scan_safe(build_chain(cfg, fs)[2], (n + 63) // 64)
        iq = S.am_tone_c64(n, fs, seed=590 + k, carrier_hz=float(cfg.offset_hz), depth=0.7)
        import torch
        d = torch.from_numpy(iq).cuda()
        par, mp = (t.cpu().numpy() for t in wh.ChannelBank(fs, n, [cfg]).process_device(d, 1))
        seq, ms = (t.cpu().numpy() for t in wh.ChannelBank(fs, n, [cfg], iir_form="sequential").process_device(d, 1))
        assert np.isfinite(par).all() and peak_rel_err(par[0, 0], seq[0, 0]) <= 5e-6, (k, peak_rel_err(par[0, 0], seq[0, 0]))
        assert abs(mp[0, 0, 1] - ms[0, 0, 1]) <= 1e-4


def test_chain_nbfm_other_rates_vs_oracle(wh, O):
    """The fused FM kernel's other shapes against the numpy oracle: odd decimation (240 kS/s -> 48 k: down 5, generic
    FIR branch), a small even one (192 kS/s: down 4, paired-tap branch with a short window), 1.2 MS/s (down 25, odd)
    and an interpolating pair (250 kS/s -> 48 k: up 24 / down 125, unfused resampler); int16 and complex64 inputs,
    several channels per bank, chunk lengths that are not multiples of the tile."""
    for fs, n in ((240_000, 12_000), (192_000, 9_613), (1_200_000, 60_000), (250_000, 12_500)):
        offs = [-fs / 5.0, 0.0, fs / 7.0]
        iq = sum(S.fm_tone_c64(n, fs, seed=600 + k, audio_hz=500.0 + 300 * k, deviation=3000.0, carrier_hz=o, noise_amp=0.01, amp=0.3)
                 for k, o in enumerate(offs)).astype(np.complex64)
        i16 = S.pack_iq16_np(iq)
        z = wh.unpack_iq16(i16)
        cfgs = [_nbfm_cfg(wh, o) for o in offs]
        for fmt, x in (("cf32", z), ("int16", i16)):
            res = wh.ChannelBank(fs, n, cfgs, input_format=fmt).process(x)
            for k, o in enumerate(offs):
                ref, met = O.process_channel_nbfm(z, fs, o)
                assert res[k][0].shape == ref.shape, (fs, k)
                assert peak_rel_err(res[k][0], ref) <= TOL, (fs, fmt, k, peak_rel_err(res[k][0], ref))
                assert db_close(res[k][1]["rssi_db"], met["rssi_db"])


def test_a14_noise_blanker(wh, golden):
    """noise_blanker (dsp/filters.py:267-343) standalone: bit-exact vs the reference (the samples kept are copied,
    the rest are zeros); even / odd lengths (np.median's two middle values), width 0, all-zero input."""
    g = golden("blanker")
    for tag in [str(t) for t in g["tags"]]:
        db, w = g[f"{tag}_args"]
        got = wh.noise_blanker(g[f"{tag}_in"], float(db), int(w))
        assert got.dtype == np.float32 and np.array_equal(got, g[f"{tag}_out"]), tag
    assert wh.noise_blanker(np.array([], dtype=np.float32)).size == 0


def test_chain_small_and_odd_chunk_lengths(wh, O):
    """Short / awkward chunk lengths through every row form (fused FM tiles larger than the chunk, IIR tiles of one
    partial 64-sample block, resampler output shorter than its taps): still the oracle's numbers."""
    fs = 2_400_000
    for n in (50, 63, 64, 65, 1000, 4097):
        iq = S.fm_tone_c64(n, fs, seed=700 + n, audio_hz=20_000.0, deviation=50_000.0, carrier_hz=100e3, noise_amp=0.05)
        a, m = wh.process_channel_dsp_stateless(iq, fs, _nbfm_cfg(wh, 100e3))
        ref, met = O.process_channel_nbfm(iq, fs, 100e3)
        assert a.shape == ref.shape and peak_rel_err(a, ref) <= TOL, ("nbfm", n, peak_rel_err(a, ref))
        a, m = wh.process_channel_dsp_stateless(iq, fs, wh.ChannelConfig(mode="wbfm", offset_hz=100e3))
        ref, met = O.process_channel_wbfm(iq, fs, 100e3)
        assert a.shape == ref.shape and peak_rel_err(a, ref) <= TOL, ("wbfm", n, peak_rel_err(a, ref))
        assert db_close(m["rssi_db"], met["rssi_db"])


@pytest.mark.parametrize("fs,bw,M", [(8_000_000, 25_000, 320), (2_400_000, 12_500, 192), (6_000_000, 12_500, 480),
                                      (10_000_000, 12_500, 800), (2_400_000, 25_000, 96), (1_000_000, 62_500, 16),
                                      (2_800_000, 100_000, 28)])
def test_a7_pfb_other_channel_counts_vs_oracle(wh, O, fs, bw, M):
    """The generic path for the channel counts other sample-rate / spacing pairs give: mixed-radix Stockham passes of
    radix 4, 2, 3 and 5 (M = 320 is the reference's own benchmark_dsp.py shape), and the direct-DFT fallback for a
    count with another prime factor (28 = 4 * 7); two calls so the carried history is exercised."""
    ch = wh.PolyphaseChannelizer(fs, bw)
    ref = O.PolyphaseChannelizer(fs, bw)
    assert ch.channel_count == M == ref.channel_count
    x = S.noise_c64(M * 120 + 17, 780 + M)
    for part in (x[:M * 70 + 5], x[M * 70 + 5:]):
        a, b = ch.process(part), ref.process(part)
        assert a.shape == b.shape and peak_rel_err(a, b) <= TOL, (M, peak_rel_err(a, b))
    assert np.array_equal(ch.arm_history, ref.arm_history)


@pytest.mark.parametrize("fs,bw,M", [(8_000_000, 25_000, 320), (1_600_000, 25_000, 64), (3_200_000, 12_500, 256),
                                      (6_400_000, 12_500, 512), (3_600_000, 12_500, 288), (2_400_000, 25_000, 96)])
def test_a7_pfb_run_kernel_equals_per_hop_kernel(wh, fs, bw, M):
    """Channel counts 64..512 with 4 | M and no kernel shaped for them take the run kernel (one wave per run of hops,
    register windows, in-place LDS passes); tune(path="per_hop") keeps the one-workgroup-per-hop kernel.  Same pass plan
    and arithmetic, so the outputs and the carried history must agree bit for bit -- cf32 and int16 input, ragged
    lengths (partial last run, odd hop counts, fewer hops than the head), four calls in a row."""
    import torch

    run = wh.PolyphaseChannelizer(fs, bw).tune(path="run")
    hop = wh.PolyphaseChannelizer(fs, bw).tune(path="per_hop")
    assert run.channel_count == M == hop.channel_count
    x = S.noise_c64(M * 700 + 99, 4000 + M, amp=0.25)
    c1 = M * 3 + 1                      # 5 hops (head only)
    c2 = c1 + M * 5 + M // 2            # 10 hops (two past the head: one short run)
    c3 = c2 + M * 333 + M // 2 + 7      # 666 hops, then the rest
    cuts = [0, c1, c2, c3, len(x)]
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        part = torch.from_numpy(x[lo:hi].copy()).cuda()
        ya, yb = run.process_device(part).clone(), hop.process_device(part).clone()
        assert ya.shape == yb.shape and torch.equal(ya, yb), (M, lo, hi)
    assert np.array_equal(run.arm_history, hop.arm_history)
    i16 = S.pack_iq16_np(x[: M * 150 + 11])
    run.reset(); hop.reset()
    part = torch.from_numpy(i16.copy()).cuda()
    assert torch.equal(run.process_device(part), hop.process_device(part))


# every channel count with a compile-time-shaped kernel (pfb_mid.hip WH_MID_CONFIGS); fs = M x 25 kHz
SHAPED = [(M * 25_000, 25_000, M) for M in (64, 80, 96, 128, 160, 192, 240, 256, 320, 384, 400, 480, 512, 640, 768, 800, 960,
                                             1280, 2048, 4096)]


def _shaped_kernel_checks(wh, O, fs, bw, M, T=9):
    """Channel counts with a kernel shaped at compile time (pfb_mid.hip; M = 320 is benchmark_dsp.py's shape): one launch
    per call does the head hops (carried history), the runs and the history update.  Checked (i) against the oracle over
    ragged calls (head only; one short run; many runs with a partial last one) to 1e-5, history bit-exact; (ii) against
    the per-hop kernel (different FFT factorisation: agreement to float32 rounding); (iii) a hop's bits do not depend on
    where the stream is cut into calls (head hops and run hops go through the same arithmetic); (iv) int16 input ==
    unpack first, bit for bit."""
    import torch

    ch = wh.PolyphaseChannelizer(fs, bw, taps_per_channel=T).tune(path="shaped")
    hop = wh.PolyphaseChannelizer(fs, bw, taps_per_channel=T).tune(path="per_hop")
    ref = O.PolyphaseChannelizer(fs, bw, taps_per_channel=T)
    assert ch.channel_count == M and ch.arms.shape == (M, T)
    big = M > 1024                      # fewer hops for the big shapes (the oracle is a Python loop per hop)
    x = S.noise_c64(M * (260 if big else 700) + 99, 4100 + M, amp=0.25)
    c1 = M * 3 + 1
    c2 = c1 + M * 5 + M // 2
    c3 = c2 + M * (120 if big else 333) + M // 2 + 7
    cuts = [0, c1, c2, c3, len(x)]
    pieces = []
    worst = 0.0
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        part = torch.from_numpy(x[lo:hi].copy()).cuda()
        ya, yb = ch.process_device(part).clone(), hop.process_device(part)
        yr = ref.process(x[lo:hi])
        assert tuple(ya.shape) == yr.shape == tuple(yb.shape)
        worst = max(worst, peak_rel_err(ya.cpu().numpy(), yr))
        assert peak_rel_err(ya.cpu().numpy(), yr) <= TOL, (M, lo, hi)
        assert peak_rel_err(ya.cpu().numpy(), yb.cpu().numpy()) <= 2e-6, (M, lo, hi)
        assert np.array_equal(ch.arm_history, ref.arm_history)
        pieces.append(ya)
    print(f"shaped M={M} T={T}: worst peak-relative error vs the oracle {worst:.2e}")
    # cut independence: a call that starts M/2 samples after the previous call's last hop continues the stream (its
    # history holds the stream's own blocks), so every hop must equal the one-call result bit for bit
    one, two = (wh.PolyphaseChannelizer(fs, bw, taps_per_channel=T) for _ in range(2))      # default dispatch
    HB, n_hops = M // 2, (400 if big else 900)
    xd = torch.from_numpy(x[: HB * (n_hops - 1) + M].copy()).cuda()
    whole = one.process_device(xd).clone()
    assert whole.shape[0] == n_hops
    h0 = 0
    for cnt in ((3, 11, 216, 170) if big else (3, 11, 516, 370)):
        seg = two.process_device(xd[h0 * HB: (h0 + cnt - 1) * HB + M])
        assert torch.equal(seg, whole[h0: h0 + cnt]), (M, h0, cnt)
        h0 += cnt
    assert np.array_equal(one.arm_history, two.arm_history)
    # int16 input
    i16 = S.pack_iq16_np(x[: M * 150 + 11])
    xq = torch.from_numpy(wh.unpack_iq16(i16)).cuda()
    a, b = (wh.PolyphaseChannelizer(fs, bw, taps_per_channel=T) for _ in range(2))
    ya = a.process_device(torch.from_numpy(i16.copy()).cuda())
    yb = b.process_device(xq)
    assert torch.equal(ya, yb) and np.array_equal(a.arm_history, b.arm_history)


@pytest.mark.parametrize("fs,bw,M", SHAPED)
def test_a7_pfb_shaped_kernel(wh, O, fs, bw, M):
    _shaped_kernel_checks(wh, O, fs, bw, M)


@pytest.mark.parametrize("M", [320, 1024])
@pytest.mark.parametrize("T", [5, 7, 13, 17])
def test_a7_pfb_shaped_kernel_other_arm_lengths(wh, O, M, T):
    """The two headline channel counts at taps_per_channel 5, 7, 13, 17 (pfb_mid.hip WH_MID_CONFIGS_T): same checks as
    at the default 9.  The oracle's filter design / filter code is generic in the arm length and pinned by the goldens
    at 9 only (no reference fixture or call site uses another length)."""
    _shaped_kernel_checks(wh, O, M * 25_000, 25_000, M, T)


@pytest.mark.parametrize("fs,bw,M,T", [(8_000_000, 25_000, 320, 5), (8_000_000, 25_000, 320, 12),
                                        (10_000_000, 9765, 1024, 6), (2_400_000, 12_500, 192, 16)])
def test_a7_pfb_other_tap_counts_vs_oracle(wh, O, fs, bw, M, T):
    """taps_per_channel is a constructor argument of the reference (channelizer.py:39, default 9).  Counts without a
    shaped instance (pfb_mid.hip: 9 everywhere, 5 / 7 / 13 / 17 at M = 320 and 1024) take the per-hop kernel -- same numbers as the oracle's
    restatement of the same design + filter code (pinned by the goldens at the default count), history carried across
    two calls."""
    ch = wh.PolyphaseChannelizer(fs, bw, taps_per_channel=T)
    ref = O.PolyphaseChannelizer(fs, bw, taps_per_channel=T)
    assert ch.channel_count == M == ref.channel_count and ch.arms.shape == ref.arms.shape == (M, T)
    x = S.noise_c64(M * 90 + 11, 880 + M + T)
    for part in (x[:M * 50 + 3], x[M * 50 + 3:]):
        a, b = ch.process(part), ref.process(part)
        assert a.shape == b.shape and peak_rel_err(a, b) <= TOL, (M, T, peak_rel_err(a, b))
    assert np.array_equal(ch.arm_history, ref.arm_history)


def test_a7_pfb_kernel_time_ring(wh):
    """wh_pfb_kernel_ms_back: the handle keeps the event pairs of its last 64 profiled launches, so a caller can time every
    launch of a run without waiting between them (bench.py reads the timed steps' kernel durations after the timed region);
    a launch further back than what was recorded is refused.  The long-call fast path runs the head / tail hops and the
    history update on the handle's side stream beside the fused kernel: checked against the shaped kernel family (which
    has no side stream) on the same calls, and for run-to-run equality."""
    import torch

    ch = wh.PolyphaseChannelizer(10_000_000, 9765)
    ch.profile(True)
    g = torch.Generator(device="cuda").manual_seed(5)
    x = torch.view_as_complex(torch.randn(1024 * 4200 + 77, 2, device="cuda", generator=g).mul_(0.5))   # > 8 groups per CU: forks
    outs = [ch.process_device(x[: 1024 * 4100 + 5]).clone(), ch.process_device(x[1024 * 4100 + 5:]).clone(), None]
    ch.process_device(x[:1024 * 50])
    t = [ch.last_kernel_ms(back=b) for b in range(3)]
    assert all(v > 0 for v in t) and t[2] > t[0]          # the long first call is further back
    with pytest.raises(RuntimeError):
        ch.last_kernel_ms(back=3)
    # the same calls through the shaped kernel family (one launch per call, no side stream): same numbers to the parity
    # tolerance (the two factor their transforms differently), same carried history exactly; and the fork path twice: same bits
    cut = 1024 * 4100 + 5
    ref = wh.PolyphaseChannelizer(10_000_000, 9765).tune(path="shaped")
    r0, r1 = ref.process_device(x[:cut]), ref.process_device(x[cut:])
    for a, b in ((outs[0], r0), (outs[1], r1)):
        assert a.shape == b.shape and float((a - b).abs().max() / b.abs().max()) <= TOL
    again = wh.PolyphaseChannelizer(10_000_000, 9765)
    assert torch.equal(again.process_device(x[:cut]), outs[0]) and torch.equal(again.process_device(x[cut:]), outs[1])
    ref.process_device(x[:1024 * 50])
    assert np.array_equal(ch.arm_history, ref.arm_history)


def test_a7_pfb_prefetch_forms_agree(wh):
    """The fused 1024-channel kernel prefetches the next group's samples either into registers or through the LDS DMA with
    counted waits, at two or three workgroups per CU: tune(prefetch=1 / 3) are the two-workgroup forms, 7 / 5 the
    three-workgroup forms (5 = the default, 0; different LDS images, 8-byte stores, a single DMA buffer for complex64, odd
    runs walked DOWNWARDS unless alt_dir=0), and the run length / run -> workgroup mapping are free parameters.  Same arithmetic, so every (format, form, run
    length, mapping) combination agrees bit for bit, ragged tail and second call included."""
    import torch

    x = S.noise_c64(1024 * 260 + 333, 77, amp=0.25)
    i16 = torch.from_numpy(S.pack_iq16_np(x)).cuda()
    xq = torch.from_numpy(wh.unpack_iq16(S.pack_iq16_np(x))).cuda()
    outs = {}
    for v, kw in (("1", {}), ("3", {}), ("0", {}), ("5", dict(hops_per_run=3, run_map=-1)), ("5b", dict(hops_per_run=7, run_map=4)),
                  ("5c", dict(hops_per_run=64, run_map=-2)), ("5d", dict(hops_per_run=5, alt_dir=0)), ("5e", dict(hops_per_run=2, run_map=2)),
                  ("7", dict(hops_per_run=2)), ("7b", dict(hops_per_run=16, run_map=1)), ("7c", dict(hops_per_run=9, alt_dir=0))):
        a = wh.PolyphaseChannelizer(10_000_000, 9765).tune(prefetch=int(v[0]), **kw)
        b = wh.PolyphaseChannelizer(10_000_000, 9765).tune(prefetch=int(v[0]), **kw)
        cut = 1024 * 150 + 512
        outs[v] = [torch.cat([a.process_device(xq[:cut]), a.process_device(xq[cut:])]),
                   torch.cat([b.process_device(i16[:2 * cut]), b.process_device(i16[2 * cut:])])]
    ref = outs["1"][0]
    assert all(torch.equal(ref, o) for v in outs for o in outs[v])


@pytest.mark.parametrize("M", [320, 1024, -1024, 256, 96, 2048, 640])
def test_a13_statistics_only_filterbank(wh, M):
    """wh_pfb_run_stats: the filterbank in statistics-only mode (last pass reduces |y|^2 in registers, no channel outputs
    written) == wh_pfb_channel_stats over the full output of the same input: {sum, sum of squares, count, min, max} per
    channel: count, min and max EXACTLY (both take p = float32(float32(re^2) + float32(im^2)) of bit-identical outputs), the
    two sums to 2e-6 relative (float32 block sums added in float64; the grouping into blocks differs between the
    kernels and is not part of the definition); history carried identically, two calls accumulate, int16 input; a channel
    count without a shaped kernel is refused."""
    import torch

    # M = 1024 has two statistics-only kernels: the tuned 1024-channel kernel's own form (the default) and the shaped
    # kernel's (M = -1024 here); each is compared with the full output of ITS kernel family -- the two factor their FFTs
    # differently, and float32 rounding differences of y become 1e-7 relative differences of |y|^2
    path = "shaped" if M != 1024 else "auto"
    M = abs(M)
    fs, bw = M * 25_000, 25_000
    g = torch.Generator(device="cuda").manual_seed(60 + M)
    n1, n2 = M // 2 * 700 + 33, M // 2 * 5 + 7
    x = torch.view_as_complex(torch.randn(n1 + n2, 2, device="cuda", generator=g).mul_(0.5))
    full, st = wh.PolyphaseChannelizer(fs, bw).tune(path=path), wh.PolyphaseChannelizer(fs, bw).tune(path=path)
    assert full.channel_count == M
    ref = None
    got = None
    for lo, hi in ((0, n1), (n1, n1 + n2)):
        y = full.process_device(x[lo:hi])
        ref = full.channel_stats_device(y, ref, accumulate=ref is not None)
        got = st.process_stats_device(x[lo:hi], got, accumulate=got is not None)
        assert np.array_equal(full.arm_history, st.arm_history)
    r, s = ref.cpu().numpy(), got.cpu().numpy()
    assert np.array_equal(r[:, 2:], s[:, 2:])
    err = float(np.max(np.abs(r[:, :2] - s[:, :2]) / r[:, :2]))
    record_margin(err, tol=2e-6)
    assert err <= 2e-6, err
    i16 = torch.from_numpy(S.pack_iq16_np(x[:n1].cpu().numpy())).cuda()
    a, b = wh.PolyphaseChannelizer(fs, bw).tune(path=path), wh.PolyphaseChannelizer(fs, bw).tune(path=path)
    r16 = a.channel_stats_device(a.process_device(i16)).cpu().numpy()
    s16 = b.process_stats_device(i16).cpu().numpy()
    assert np.array_equal(r16[:, 2:], s16[:, 2:]) and np.max(np.abs(r16[:, :2] - s16[:, :2]) / r16[:, :2]) <= 2e-6
    if M == 320:
        odd = wh.PolyphaseChannelizer(2_800_000, 100_000)      # M = 28: no shaped kernel
        with pytest.raises(RuntimeError):
            odd.process_stats_device(x[:28 * 50])


def test_a13_stats_merge_kernel(wh):
    """wh_stats_merge (the device half of the cross-stream activity reduction: gathered [ranks][M][5] -> [M][5]) equals the
    host merge of scanner_reduce bit for bit, for 1, 2 and 8 ranks."""
    import torch
    from wavehip.scanner_reduce import AsyncStatsReducer

    g = torch.Generator(device="cuda").manual_seed(9)
    for R in (1, 2, 8):
        x = torch.rand((R, 1024, 5), dtype=torch.float64, device="cuda", generator=g) * 1e3
        dev = AsyncStatsReducer.merge_gathered(x)
        host = AsyncStatsReducer.merge_gathered(x.cpu())
        # fixed rank order on the device; torch's host sum over dim 0 adds in the same order for these sizes
        assert dev.shape == (1024, 5) and torch.allclose(dev.cpu(), host, rtol=1e-15, atol=0)
        assert torch.equal(dev[:, 3].cpu(), host[:, 3]) and torch.equal(dev[:, 4].cpu(), host[:, 4])


def test_diag_stream_yardstick_copies_twice(wh):
    """wh_diag_stream_1r2w (the no-arithmetic traffic yardstick bench.py times beside the filterbank) really moves the
    bytes it is credited with: the input appears twice in the output, ragged length included; odd n is refused."""
    import torch
    from wavehip import _lib

    for n in (2, 1000, 4096 * 3 + 6, 1 << 20):
        x = torch.view_as_complex(torch.randn(n, 2, device="cuda"))
        y = torch.zeros(2 * n, dtype=torch.complex64, device="cuda")
        _lib.check(_lib.lib.wh_diag_stream_1r2w(x.data_ptr(), y.data_ptr(), n, _lib.stream_ptr(torch)), "diag")
        torch.cuda.synchronize()
        assert torch.equal(y[:n], x) and torch.equal(y[n:], x)
    assert _lib.lib.wh_diag_stream_1r2w(x.data_ptr(), y.data_ptr(), 3, None) != 0
    for n in (2, 4096 * 3 + 6):                      # the 1 : 4 form (the int16-input filterbank's traffic shape)
        x = torch.view_as_complex(torch.randn(n, 2, device="cuda"))
        y = torch.zeros(4 * n, dtype=torch.complex64, device="cuda")
        _lib.check(_lib.lib.wh_diag_stream_1r4w(x.data_ptr(), y.data_ptr(), n, _lib.stream_ptr(torch)), "diag")
        torch.cuda.synchronize()
        assert all(torch.equal(y[k * n:(k + 1) * n], x) for k in range(4))


def test_operator_from_a_thread_pool(wh, golden):
    """The reference calls _process_channel_dsp_stateless from a ThreadPoolExecutor(max_workers=3)
    (capture.py:1906-1925, 2521-2567): the drop-in must give the same results when 3 threads hammer it with
    different channels of the same chunk (shared bank cache, per-bank workspace)."""
    from concurrent.futures import ThreadPoolExecutor
    g = golden("chain_analog")
    fs, n, seed0 = (int(v) for v in g["nbfm_args"])
    offs = S.nbfm_bank_offsets()
    z = wh.unpack_iq16(S.pack_iq16_np(S.nbfm_bank_c64(n, fs, seed=seed0, start=0)))
    ks = [0, 13, 31, 5, 20, 13, 0, 31]
    serial = [wh.process_channel_dsp_stateless(z, fs, _nbfm_cfg(wh, offs[k])) for k in ks]
    with ThreadPoolExecutor(max_workers=3) as ex:
        for _ in range(3):
            par = list(ex.map(lambda k: wh.process_channel_dsp_stateless(z, fs, _nbfm_cfg(wh, offs[k])), ks))
            for a, b in zip(serial, par):
                assert np.array_equal(a[0], b[0]) and a[1] == b[1]
    for k, r in zip(ks, serial):
        if k in (0, 13, 31):
            assert peak_rel_err(r[0], g[f"nbfm0_k{k}_audio"]) <= TOL
