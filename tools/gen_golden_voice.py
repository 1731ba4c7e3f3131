#!/usr/bin/env python3
"""Golden vectors for the voice-recorder symbol path (wavehip.voice), made by importing the real WaveCap-SDR reference.

Runs ONLY on the build machine, on the CPU (it needs the reference's sources; no GPU test, smoke() or bench.py reads
the reference or this script).  Writes

    tests/golden/voice.npz           DiscriminatorDemodulator (decoders/p25.py:1105-1345) on 48 / 50 kHz disc audio
    tests/golden/voice_recorder.npz  VoiceRecorder.process_iq (trunking/system.py:500-790) -> discriminator ->
                                     P25Decoder.process_discriminator -> DiscriminatorDemodulator.demodulate

Usage:  cd /tmp && PYTHONDONTWRITEBYTECODE=1 python3 <repo>/tools/gen_golden_voice.py [reference backend dir]

Case selection (the slicer's timing loop quantises mu to 1/128 and is chaotic under 1-ulp changes, so a case is kept
as a bit-exact golden only when the REFERENCE's own dibits do not move under the perturbations the device introduces):
  (a) np.convolve replaced by a float64-accumulated convolution rounded to float32 (the device's low-pass);
  (b) chained cases: the decimated IQ rounded to complex64 before np.angle (the device's DDC writes complex64);
  (c) N_ULP_DRAWS draws of independent +-1-ulp noise on the disc audio (float64 angle / unwrap rounding).
Seeds are tried in order for every case; the counts of seeds tried and kept are printed and stored.
"""

from __future__ import annotations

import contextlib
import logging
import os
import sys

REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference/backend"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.dont_write_bytecode = True
sys.path.insert(0, REF)
sys.path.insert(0, os.path.join(REPO, "tests"))

import numpy as np  # noqa: E402
import scipy  # noqa: E402

import signals as S  # noqa: E402

import wavecapsdr.trunking  # noqa: E402,F401  (must precede the decoders: circular import)
from wavecapsdr.decoders import p25 as rp25  # noqa: E402
from wavecapsdr.trunking import system as rsys  # noqa: E402

logging.disable(logging.CRITICAL)    # the recorder logs every chunk
GOLD = os.path.join(REPO, "tests", "golden")
META = dict(numpy=np.__version__, scipy=scipy.__version__)
N_ULP_DRAWS = 3
MAX_SEEDS = 40
VARS = ("_symbol_clock", "_symbol_spread", "_dc_estimate", "_fine_freq_correction", "_coarse_freq_correction",
        "_input_gain")


def save(name, **kw):
    kw["meta"] = np.array(repr(META))
    path = os.path.join(GOLD, name + ".npz")
    np.savez_compressed(path, **kw)
    print(f"{name}: {os.path.getsize(path) / 1024:.1f} KiB")


def state_of(d):
    """values (float64), float32 flags, history ring, history index, symbol count"""
    vals = [float(getattr(d, v)) for v in VARS]
    flags = []
    for v in VARS:
        x = getattr(d, v)
        assert isinstance(x, (float, np.float32)) and not isinstance(x, np.float64), (v, type(x))
        flags.append(int(isinstance(x, np.float32)))
    return vals, flags, d._history.copy(), d._history_idx, d._symbol_count


@contextlib.contextmanager
def f64_convolve():
    real = np.convolve

    def conv(a, v, mode="full"):
        a, v = np.asarray(a), np.asarray(v)
        if a.dtype != np.float32 or v.dtype != np.float32:     # only the demodulator's float32 low-pass is replaced
            return real(a, v, mode)
        return real(a.astype(np.float64), v.astype(np.float64), mode).astype(np.float32)

    np.convolve = conv
    try:
        yield
    finally:
        np.convolve = real


def ulp_noise(x, rng):
    x = np.asarray(x, dtype=np.float32)
    s = rng.integers(-1, 2, size=x.size)
    return np.where(s > 0, np.nextafter(x, np.float32(np.inf)),
                    np.where(s < 0, np.nextafter(x, np.float32(-np.inf)), x)).astype(np.float32)


# ---------------------------------------------------------------- standalone DiscriminatorDemodulator

def disc_audio(n, fs, seed, snr_db):
    """48 kHz discriminator audio of the C4FM test signal (the recorder's angle / unwrap / diff), float32."""
    iq = S.c4fm_iq(n + 1, fs, seed, snr_db=snr_db, freq_offset_hz=60.0)[0].astype(np.complex128)
    return np.diff(np.unwrap(np.angle(iq))).astype(np.float32)


def run_standalone(fs, calls, resets, perturb=None, conv64=False):
    d = rp25.DiscriminatorDemodulator(sample_rate=fs)
    dib, cnt, states = [], [], []
    ctx = f64_convolve() if conv64 else contextlib.nullcontext()
    with ctx:
        for k, x in enumerate(calls):
            if k in resets:
                d.reset()
            y = perturb(x) if perturb is not None else x
            out = d.demodulate(y)
            dib.append(out)
            cnt.append(len(out))
            states.append(state_of(d))
    return np.concatenate(dib).astype(np.uint8), np.array(cnt, dtype=np.int64), states, d


def stable(fs, calls, resets, base, rng):
    """-> the states under perturbation (a) when the dibits survive every perturbation, else None"""
    dib64, _, states64, _ = run_standalone(fs, calls, resets, conv64=True)
    if not np.array_equal(dib64, base):
        return None
    for _ in range(N_ULP_DRAWS):
        if not np.array_equal(run_standalone(fs, calls, resets, perturb=lambda x: ulp_noise(x, rng))[0], base):
            return None
    return states64


STANDALONE = [
    # name, sample rate, SNR dB (None: noise only; 0: all zero), DC offset, form, call lengths, resets before call k
    ("snr25_dc+", 48000, 25.0, 0.2, "f32", [50, 80, 4800, 7200, 100, 101, 65, 64, 4800, 99, 2400], ()),
    ("snr12_dc-", 48000, 12.0, -0.2, "f32", [4800, 30, 4800, 7200, 66, 4800], ()),
    ("snr25_i16", 48000, 25.0, 0.0, "i16", [4800, 7200, 4800, 90, 4800], ()),
    ("noise_reset", 48000, None, 0.0, "f32", [4800, 4800, 70, 4800, 4800], (3,)),
    ("zeros", 48000, 0, 0.0, "f32", [4800, 50, 7200, 4800], ()),
    ("long72k", 48000, 25.0, 0.0, "i16", [72000], ()),
    ("fs50k", 50000, 25.0, 0.1, "f32", [5000, 77, 5000, 7500, 5000], (2,)),
]


def gen_standalone(out):
    kept_total = tried_total = 0
    out["bb_taps"] = rp25.DiscriminatorDemodulator(48000)._baseband_taps
    out["bb_taps_50k"] = rp25.DiscriminatorDemodulator(50000)._baseband_taps
    out["mmse"] = rp25.DiscriminatorDemodulator(48000)._mmse_taps
    for ci, (name, fs, snr, dc, form, lens, resets) in enumerate(STANDALONE):
        n = sum(lens)
        for si in range(MAX_SEEDS):
            seed = 4100 + 37 * ci + si
            tried_total += 1
            if snr is None:
                rng = np.random.default_rng(seed)
                x = (rng.uniform(-np.pi, np.pi, n)).astype(np.float32)
            elif snr == 0:
                x = np.zeros(n, dtype=np.float32)
            else:
                x = (disc_audio(n, fs, seed, snr) + np.float32(dc)).astype(np.float32)
            if form == "i16":
                raw = np.clip(np.round(x * 8000.0), -32768, 32767).astype(np.int16)
                x = raw.astype(np.float32) / 32768.0       # process_discriminator's int16 rule (p25.py:2354-2355)
                stored = raw
            else:
                stored = x
            calls = np.split(x, np.cumsum(lens)[:-1])
            base, cnt, states, _ = run_standalone(fs, calls, set(resets))
            states64 = stable(fs, calls, set(resets), base, np.random.default_rng(seed + 1))
            if states64 is None:
                print(f"  {name}: seed {seed} not stable, next")
                continue
            kept_total += 1
            print(f"  {name}: seed {seed} kept after {si + 1} tries ({len(base)} dibits)")
            out[f"k{ci}_name"] = np.array(name)
            out[f"k{ci}_rate"] = np.array(fs, dtype=np.int64)
            out[f"k{ci}_seed"] = np.array(seed, dtype=np.int64)
            out[f"k{ci}_tries"] = np.array(si + 1, dtype=np.int64)
            out[f"k{ci}_audio"] = stored
            out[f"k{ci}_lens"] = np.array(lens, dtype=np.int64)
            out[f"k{ci}_resets"] = np.array(list(resets) + [-1], dtype=np.int64)
            out[f"k{ci}_dibits"] = base
            out[f"k{ci}_counts"] = cnt
            out[f"k{ci}_vals"] = np.array([s[0] for s in states], dtype=np.float64)
            out[f"k{ci}_flags"] = np.array([s[1] for s in states], dtype=np.int64)
            out[f"k{ci}_hist"] = np.array([s[2] for s in states], dtype=np.float32)
            out[f"k{ci}_hidx"] = np.array([s[3] for s in states], dtype=np.int64)
            out[f"k{ci}_symcount"] = np.array([s[4] for s in states], dtype=np.int64)
            # the same run with the low-pass accumulated in float64 (perturbation (a) = the device's low-pass): numpy's
            # float32 convolve sums through the BLAS's sdot, whose order depends on the CPU, so the filtered samples and
            # the float32 loop state are bit-reproducible only against this run; the dibits are the same by selection
            assert [s[1] for s in states64] == [s[1] for s in states] and [s[3:] for s in states64] == [s[3:] for s in states]
            out[f"k{ci}_vals_f64lpf"] = np.array([s[0] for s in states64], dtype=np.float64)
            out[f"k{ci}_hist_f64lpf"] = np.array([s[2] for s in states64], dtype=np.float32)
            break
        else:
            raise SystemExit(f"{name}: no stable seed in {MAX_SEEDS}")
    out["n_cases"] = np.array(len(STANDALONE))
    print(f"standalone: {tried_total} seeds tried, {kept_total} kept")
    return tried_total, kept_total


# ---------------------------------------------------------------- chained VoiceRecorder cases

FS, CHUNK = 6_000_000, 150_000


def recorder_input(seed, n_chunks):
    """two C4FM carriers 1.2375 MHz apart (the trunk_recorder recipe), then an all-zero chunk and a NaN chunk"""
    n = n_chunks * CHUNK
    x = S.c4fm_iq(n, FS, seed, snr_db=25.0, freq_offset_hz=412_500.0)[0]
    x = (x + np.roll(x, 7) * np.exp(-2j * np.pi * 1_237_500.0 * np.arange(x.size) / FS)).astype(np.complex64)
    return x


# per chunk: (kind, [(recorder, offset or None = idle / "assign:<offset>" = reassigned before this chunk)])
OFFSETS = (412_500.0, -825_000.0, 2_990_000.0)      # recorder 2 is outside the +-(fs/2 - 50 kHz) band: skipped
PLAN = [
    ("data", (1, 1, 1)),
    ("data", (1, 0, 1)),            # recorder 1 idle for one chunk
    ("zero", (1, 1, 1)),            # muted chunk: signed zeros reach np.angle
    ("data", (1, 1, 1)),
    ("nan", (1, 1, 1)),             # non-finite chunk: every recorder drops it, state unchanged
    ("data", (1, 1, 1)),
    ("data", (1, 1, 1)),            # recorder 0 reassigned to 412.5 kHz - 37.5 kHz before this chunk
]
REASSIGN = {6: (0, 375_000.0)}


def make_recorder(rid, offset):
    r = rsys.VoiceRecorder(id=rid, system_id="s")
    r.setup_decimation_filter(FS, 48000)
    assign(r, offset)
    return r


def assign(r, offset):
    """VoiceRecorder.assign's DSP resets (system.py:386-393) + start_voice_channel's new P25Decoder (:446)"""
    r.offset_hz = offset
    r._last_phase = 0.0
    r._stage1_filter_zi = None
    r._stage2_filter_zi = None
    r._freq_shift_sample_idx = 0
    r._freq_shift_last_offset_hz = 0.0
    r.state = "recording"
    r._voice_channel = object()      # only tested for None before the DSP
    r._p25_decoder = rp25.P25Decoder(sample_rate=48000)


def run_chained(x, iq_round=False, conv64=False, disc_perturb=None):
    recs = [make_recorder(f"r{k}", OFFSETS[k]) for k in range(3)]
    res = {k: dict(disc=[], dib=[], cnt=[], phase=[], called=[]) for k in range(3)}
    real_angle = np.angle
    real_pd = rp25.P25Decoder.process_discriminator
    real_dm = rp25.DiscriminatorDemodulator.demodulate
    box = {}

    def angle(z, deg=False):
        if iq_round:
            z = np.asarray(z).astype(np.complex64).astype(np.complex128)
        return real_angle(z, deg)

    def pd(self, audio, sample_rate=48000):
        box["disc"] = np.asarray(audio).copy()
        if disc_perturb is not None:
            audio = disc_perturb(audio)
        return real_pd(self, audio, sample_rate)

    def dm(self, audio):
        o = real_dm(self, audio)
        box["dib"] = o.copy()
        return o

    rsys.np.angle = angle
    rp25.P25Decoder.process_discriminator = pd
    rp25.DiscriminatorDemodulator.demodulate = dm
    ctx = f64_convolve() if conv64 else contextlib.nullcontext()
    try:
        with ctx:
            pos = 0
            for ci, (kind, act) in enumerate(PLAN):
                chunk = x[pos:pos + CHUNK]
                pos += CHUNK
                if kind == "zero":
                    chunk = np.zeros(CHUNK, dtype=np.complex64)
                elif kind == "nan":
                    chunk = chunk.copy()
                    chunk[CHUNK // 3] = np.nan
                if ci in REASSIGN:
                    k, off = REASSIGN[ci]
                    assign(recs[k], off)
                for k, r in enumerate(recs):
                    if not act[k]:
                        res[k]["called"].append(0)
                        continue
                    box.clear()
                    try:
                        r.process_iq(chunk, FS)
                    except Exception:   # the vocoder hand-off after the demodulator has no event loop here
                        pass
                    called = "dib" in box
                    res[k]["called"].append(int(called))
                    if called:
                        res[k]["disc"].append(box["disc"].astype(np.float32))
                        res[k]["dib"].append(box["dib"].astype(np.uint8))
                        res[k]["cnt"].append(len(box["dib"]))
                    res[k]["phase"].append(float(r._last_phase))
    finally:
        rsys.np.angle = real_angle
        rp25.P25Decoder.process_discriminator = real_pd
        rp25.DiscriminatorDemodulator.demodulate = real_dm
    return res


def gen_chained(out):
    tried = kept = 0
    for si in range(MAX_SEEDS):
        seed = 1210 + si
        tried += 1
        x = recorder_input(seed, len(PLAN))
        base = run_chained(x)

        def dibs(r):
            return [np.concatenate(r[k]["dib"]) if r[k]["dib"] else np.zeros(0, np.uint8) for k in range(3)]

        want = dibs(base)
        ok = all(np.array_equal(a, b) for a, b in zip(dibs(run_chained(x, iq_round=True)), want))
        ok = ok and all(np.array_equal(a, b) for a, b in zip(dibs(run_chained(x, conv64=True)), want))
        rng = np.random.default_rng(seed + 1)
        for _ in range(N_ULP_DRAWS):
            if not ok:
                break
            ok = all(np.array_equal(a, b) for a, b in zip(
                dibs(run_chained(x, disc_perturb=lambda a: ulp_noise(a, rng))), want))
        if not ok:
            print(f"  chained: seed {seed} not stable, next")
            continue
        kept += 1
        print(f"  chained: seed {seed} kept after {si + 1} tries ({[len(v) for v in want]} dibits)")
        out["seed"] = np.array(seed, dtype=np.int64)
        out["sha"] = np.array(S.sha256(x))
        out["fs"] = np.array(FS, dtype=np.int64)
        out["chunk"] = np.array(CHUNK, dtype=np.int64)
        out["offsets"] = np.array(OFFSETS)
        out["plan_kind"] = np.array([p[0] for p in PLAN])
        out["plan_active"] = np.array([p[1] for p in PLAN], dtype=np.int64)
        out["reassign"] = np.array([[ci, k, off] for ci, (k, off) in REASSIGN.items()], dtype=np.float64)
        for k in range(3):
            r = base[k]
            out[f"r{k}_called"] = np.array(r["called"], dtype=np.int64)
            out[f"r{k}_disc"] = np.concatenate(r["disc"]) if r["disc"] else np.zeros(0, np.float32)
            out[f"r{k}_disc_lens"] = np.array([len(v) for v in r["disc"]], dtype=np.int64)
            out[f"r{k}_dibits"] = want[k]
            out[f"r{k}_counts"] = np.array(r["cnt"], dtype=np.int64)
            out[f"r{k}_phase"] = np.array(r["phase"], dtype=np.float64)
        break
    else:
        raise SystemExit(f"chained: no stable seed in {MAX_SEEDS}")
    print(f"chained: {tried} seeds tried, {kept} kept")
    return tried, kept


def main():
    out = {}
    t, k = gen_standalone(out)
    out["seeds_tried"], out["seeds_kept"] = np.array(t), np.array(k)
    save("voice", **out)
    out = {}
    t, k = gen_chained(out)
    out["seeds_tried"], out["seeds_kept"] = np.array(t), np.array(k)
    save("voice_recorder", **out)


if __name__ == "__main__":
    main()
