"""Front of a live P25 channel on the MI355X: capture.py:2619-2700 runs, per chunk and channel,

    wideband chunk -> freq_shift(iq, offset, fs) -> decimate_iq_for_p25(base, fs) -> P25Decoder(p25_rate).process_iq

`P25ChannelFront` does the first two steps for n channels that share one wideband chunk on the device (one launch per
64 channels, libwavehip's wh_p25front).  `P25ChannelBank` chains it into the existing symbol banks at the returned rate
(`LSMBank` for LSM, the reference's default modulation, `C4FMBank` for C4FM) and produces the framer's soft symbols, so
`SoftSyncBank` / `P25NIDFrontEnd` can run without the chunk leaving the device.  `decimate_iq_for_p25` is the host
drop-in for capture.py:203.

decimate_iq_for_p25's plan (g = gcd(fs, 48000), up = 48000 / g, down = fs / g):
  fs <= 48000: pass-through; down > 50: iq[::fs // 48000] at fs // D; otherwise scipy.signal.resample_poly(., up, down)
  on both rails at fs * up // down.  With float32 rails scipy designs the taps in float32 and accumulates in float32;
  the kernel repeats that arithmetic in scipy's order."""

from __future__ import annotations

import ctypes as C
from math import gcd

import numpy as np
from scipy import signal

from . import _lib
from .c4fm import C4FMBank
from .lsm import LSMBank

TARGET_RATE = 48000          # decimate_iq_for_p25's TARGET_RATE
SUBSAMPLE_ABOVE = 50         # down > 50 -> plain subsampling
MIN_SAMPLE_RATE = 19200      # P25Decoder.MIN_SAMPLE_RATE: below it the decoder upsamples (out of scope here)
MAX_SAMPLES = 1 << 24        # the float32 sample index of freq_shift is exact up to here
DIBIT_TO_SOFT = (1.0, 3.0, -1.0, -3.0)   # decoders/p25.py:1942-1948, demodulators without demodulate_soft


def p25_plan(sample_rate: int) -> dict:
    """decimate_iq_for_p25's branch for `sample_rate`: kind ("pass", "subsample", "resample"), up, down, the
    subsample step D and the output rate."""
    fs = int(sample_rate)
    if fs <= 0:
        raise ValueError(f"sample_rate must be positive, got {sample_rate}")
    if fs <= TARGET_RATE:
        return dict(kind="pass", up=1, down=1, step=1, rate=fs)
    g = gcd(fs, TARGET_RATE)
    up, down = TARGET_RATE // g, fs // g
    if down > SUBSAMPLE_ABOVE:
        d = fs // TARGET_RATE
        return dict(kind="subsample", up=up, down=down, step=d, rate=fs // d)
    return dict(kind="resample", up=up, down=down, step=down, rate=(fs * up) // down)


def resample_poly_taps(up: int, down: int) -> np.ndarray:
    """The taps scipy.signal.resample_poly uses for a float32 signal: firwin(2*10*max + 1, 1/max, ("kaiser", 5.0))
    cast to float32, then multiplied by up in float32."""
    max_rate = max(up, down)
    h = signal.firwin(2 * 10 * max_rate + 1, 1.0 / max_rate, window=("kaiser", 5.0)).astype(np.float32)
    h *= up
    return np.ascontiguousarray(h)


def out_len(n: int, sample_rate: int) -> int:
    """Samples decimate_iq_for_p25 returns for a chunk of n."""
    p = p25_plan(sample_rate)
    if p["kind"] == "resample":
        nu = n * p["up"]
        return nu // p["down"] + bool(nu % p["down"])
    return -(-n // p["step"])


class P25ChannelFront(_lib.Handle):
    """freq_shift + decimate_iq_for_p25 for n_channels channels of one wideband chunk.  Stateless per call, as the
    reference: every chunk is shifted from sample index 0 and resampled with zero padding at both ends."""

    _growth = 1.5

    def __init__(self, n_channels: int, sample_rate: int, max_samples_per_call: int = 1 << 18):
        if int(n_channels) < 1:
            raise ValueError(f"n_channels must be >= 1, got {n_channels}")
        if not 1 <= int(max_samples_per_call) <= MAX_SAMPLES:
            raise ValueError(f"max_samples_per_call must be in [1, 2^24], got {max_samples_per_call}")
        self.plan = p25_plan(sample_rate)
        self._torch = _lib.require_gpu()
        self.n_channels, self.sample_rate = int(n_channels), int(sample_rate)
        self.output_rate = self.plan["rate"]
        self.taps = (resample_poly_taps(self.plan["up"], self.plan["down"]) if self.plan["kind"] == "resample"
                     else None)
        self._create("wh_p25front", self.n_channels, self.sample_rate,
                     None if self.taps is None else _lib.dptr(self.taps, "f32"),
                     0 if self.taps is None else len(self.taps))
        self.offsets_hz = np.zeros(self.n_channels, dtype=np.float64)
        self._out = None
        self.max_samples_per_call = 0
        self.reserve(int(max_samples_per_call))

    def out_len(self, n: int) -> int:
        return int(_lib.lib.wh_p25front_out_len(self._h, int(n)))

    def reserve(self, max_samples_per_call: int) -> None:
        """Size the output buffer for chunks of up to `max_samples_per_call` samples (a longer chunk does it itself)."""
        if max_samples_per_call <= self.max_samples_per_call:
            return
        if not 1 <= max_samples_per_call <= MAX_SAMPLES:
            raise ValueError(f"max_samples_per_call must be in [1, 2^24], got {max_samples_per_call}")
        self.max_samples_per_call = int(max_samples_per_call)
        self._out = self._torch.zeros((self.n_channels, max(1, self.out_len(self.max_samples_per_call))),
                                      dtype=self._torch.complex64, device="cuda")

    def set_offsets(self, offsets_hz) -> None:
        offs = np.ascontiguousarray(offsets_hz, dtype=np.float64)
        if offs.shape != (self.n_channels,):
            raise ValueError(f"offsets_hz must have shape ({self.n_channels},), got {offs.shape}")
        if not np.all(np.isfinite(offs)):
            raise ValueError("offsets_hz must be finite")
        _lib.check(_lib.lib.wh_p25front_set_offsets(self._h, _lib.dptr(offs, "f64")), "wh_p25front_set_offsets")
        self.offsets_hz[:] = offs

    def _mask(self, active):
        if active is None:
            return None
        act = np.ascontiguousarray(np.asarray(active, dtype=bool), dtype=np.uint8)
        if act.shape != (self.n_channels,):
            raise ValueError(f"active must have shape ({self.n_channels},), got {act.shape}")
        return act

    def process_device(self, iq_dev, offsets_hz=None, active=None):
        """iq_dev complex64 GPU tensor [n] -> (iq_out complex64 [N, m] view of the front's buffer, output rate).
        Rows of inactive channels are left as they were.  The buffer is overwritten by the next call."""
        torch = self._torch
        if not (isinstance(iq_dev, torch.Tensor) and iq_dev.is_cuda and iq_dev.dtype == torch.complex64
                and iq_dev.dim() == 1 and iq_dev.is_contiguous()):
            raise ValueError("iq_dev must be a contiguous 1-D complex64 GPU tensor")
        if offsets_hz is not None:
            self.set_offsets(offsets_hz)
        act = self._mask(active)
        n = iq_dev.numel()
        if n > MAX_SAMPLES:
            raise ValueError(f"chunk of {n} samples exceeds 2^24")
        if n > self.max_samples_per_call:
            self.reserve(min(MAX_SAMPLES, max(n, int(self.max_samples_per_call * self._growth))))
        m = self.out_len(n)
        _lib.check(_lib.lib.wh_p25front_run(self._h, iq_dev.data_ptr(), n, None if act is None else act.ctypes.data,
                                            self._out.data_ptr(), self._out.shape[1], _lib.stream_ptr(torch)),
                   "wh_p25front_run")
        return self._out[:, :m], self.output_rate

    def process(self, iq, offsets_hz=None, active=None) -> tuple[np.ndarray, int]:
        """Host form: iq complex64 [n] -> (complex64 [N, m], rate)."""
        x = np.ascontiguousarray(iq, dtype=np.complex64).reshape(-1)
        if x.size == 0:
            if offsets_hz is not None:
                self.set_offsets(offsets_hz)
            return np.zeros((self.n_channels, 0), dtype=np.complex64), self.output_rate
        out, rate = self.process_device(self._torch.from_numpy(x).cuda(), offsets_hz, active)
        return out.cpu().numpy(), rate


_FRONTS: dict[int, P25ChannelFront] = {}


def decimate_iq_for_p25(iq, sample_rate: int) -> tuple[np.ndarray, int]:
    """Drop-in for capture.py:203 decimate_iq_for_p25 (host arrays in and out, the work on the device).  The
    pass-through branch and an empty chunk return `iq` itself, as the reference does."""
    fs = int(sample_rate)
    if fs <= TARGET_RATE or np.asarray(iq).size == 0:
        return iq, fs
    f = _FRONTS.get(fs)
    if f is None:
        f = _FRONTS[fs] = P25ChannelFront(1, fs)
    out, rate = f.process(iq)
    return out[0], rate


class P25ChannelBank:
    """n_channels live Phase-1 P25 channels on one wideband chunk: P25ChannelFront -> LSMBank / C4FMBank at the front's
    output rate (P25Decoder uses that rate directly when it is >= 19 200 Hz) -> dibits and the framer's soft symbols.

    process_device(iq_dev, offsets_hz, active) -> (dibits uint8 [N, cap], soft float32 [N, cap], counts int32 [N]) on
    the device, or None when the chunk is empty or not finite (the capture path drops such a chunk before any state
    moves, capture.py:2621-2646).  The one host synchronisation per chunk is that finiteness check.

    The symbol banks advance every channel on every call; they have no per-channel mask or reset.  An inactive channel
    therefore gets a zero row and a count of 0, and its demodulator is not held: `reset()` (all channels) before such a
    channel is used again."""

    MODULATIONS = ("lsm", "c4fm")

    def __init__(self, n_channels: int, sample_rate: int, modulation: str = "lsm",
                 max_samples_per_call: int = 1 << 18):
        if modulation not in self.MODULATIONS:
            raise ValueError(f"modulation must be one of {self.MODULATIONS} (Phase 2 is not supported), got "
                             f"{modulation!r}")
        if int(n_channels) < 1:
            raise ValueError(f"n_channels must be >= 1, got {n_channels}")
        plan = p25_plan(sample_rate)
        if plan["rate"] < MIN_SAMPLE_RATE:
            raise ValueError(f"sample rate {sample_rate} gives a P25 rate of {plan['rate']} Hz < {MIN_SAMPLE_RATE}: "
                             "P25Decoder would upsample, which is not supported")
        self._torch = _lib.require_gpu()
        self.n_channels, self.sample_rate, self.modulation = int(n_channels), int(sample_rate), modulation
        self.front = P25ChannelFront(n_channels, sample_rate, max_samples_per_call)
        self.p25_rate = self.front.output_rate
        m = max(1, self.front.out_len(max_samples_per_call))
        if modulation == "lsm":
            self.demod = LSMBank(self.n_channels, self.p25_rate, max_samples_per_call=m)
        else:
            self.demod = C4FMBank(self.n_channels, self.p25_rate, max_samples_per_call=m)
        self._lut = self._torch.tensor(DIBIT_TO_SOFT, dtype=self._torch.float32, device="cuda")
        self._soft = None

    def reset(self, channel: int = -1) -> None:
        """A fresh demodulator for every channel.  channel >= 0 is refused: the symbol banks reset as a whole."""
        if channel != -1:
            raise ValueError("P25ChannelBank.reset: the symbol banks reset all channels together; use channel=-1")
        self.demod.reset()

    def process_device(self, iq_dev, offsets_hz=None, active=None):
        torch = self._torch
        if offsets_hz is not None:
            self.front.set_offsets(offsets_hz)
        act = self.front._mask(active)
        if iq_dev.numel() == 0:
            return None
        if not bool(torch.isfinite(torch.view_as_real(iq_dev)).all()):   # the one host synchronisation
            return None
        base, _ = self.front.process_device(iq_dev, None, act)
        if act is not None and not act.all():
            base[torch.from_numpy(act == 0).to(base.device)] = 0
        if self.modulation == "lsm":
            dib, _, cnt = self.demod.demodulate_device(base)
            if self._soft is None or self._soft.shape != dib.shape:
                self._soft = torch.empty(dib.shape, dtype=torch.float32, device=dib.device)
            # rows hold counts[c] dibits; the entries after them are stale bytes: & 3 keeps every index inside the map
            torch.take(self._lut, (dib & 3).long(), out=self._soft)
            soft = self._soft
        else:
            dib, soft, cnt = self.demod.demodulate_device(base)
        if act is not None:
            cnt = cnt * torch.from_numpy(act.astype(np.int32)).to(cnt.device)
        return dib, soft, cnt

    def process(self, iq, offsets_hz=None, active=None) -> list:
        """Host form -> per channel (dibits uint8, soft float32), or None for an inactive channel or a dropped chunk."""
        x = np.ascontiguousarray(iq, dtype=np.complex64).reshape(-1)
        r = None if x.size == 0 else self.process_device(self._torch.from_numpy(x).cuda(), offsets_hz, active)
        if r is None:
            if x.size == 0 and offsets_hz is not None:
                self.front.set_offsets(offsets_hz)
            return [None] * self.n_channels
        dib, soft, cnt = r
        cnt = cnt.cpu().numpy()
        mx = int(cnt.max()) if cnt.size else 0
        d, s = dib[:, :mx].cpu().numpy(), soft[:, :mx].cpu().numpy()
        out = []
        for k in range(self.n_channels):
            if active is not None and not active[k]:
                out.append(None)
            else:
                out.append((d[k, :cnt[k]].copy(), s[k, :cnt[k]].copy()))
        return out
