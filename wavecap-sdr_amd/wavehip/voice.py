"""Voice-recorder symbol path on the MI355X: FM discriminator + DiscriminatorDemodulator bank.

`DiscriminatorDemodulator` is the drop-in for wavecapsdr.decoders.p25.DiscriminatorDemodulator (p25.py:1105-1345:
ctor `(sample_rate=48000, symbol_rate=4800)`, `demodulate(audio) -> dibits uint8`, `reset()`), over a one-channel
`DiscriminatorBank`.  One `demodulate` call = one reference call: the auto-gain is per call and the 'same'-mode
low-pass re-seeds on every call, so where a stream is cut is part of the result and calls are never split.

`VoiceRecorderBank` is the DSP of VoiceRecorder.process_iq (trunking/system.py:500-790) for a pool of recorders on one
wideband buffer: `TrunkingDDCBank(plan="recorder")` -> decimated 48 kHz IQ -> discriminator with the carried unwrapped
phase (:708-717) -> DiscriminatorDemodulator (P25Decoder.process_discriminator, p25.py:2323-2361), all on the device.

Deliberate difference: a call with 0 decimated samples is a no-op here; the reference raises on it
(disc_audio.min() of an empty array, system.py:722)."""

from __future__ import annotations

import ctypes as C

import numpy as np
from scipy import signal

from . import _lib
from .trunking import TrunkingDDCBank

BASEBAND_CUTOFF_HZ = 5200
BASEBAND_TAPS = 65
MMSE_NTAPS = 8
MMSE_NSTEPS = 128
STATE_VARS = ("symbol_clock", "symbol_spread", "dc_estimate", "fine_freq_correction", "coarse_freq_correction",
              "input_gain")


def design_baseband_filter(sample_rate: float) -> np.ndarray:
    """p25.py:1201-1208: 65-tap Hamming firwin at 5.2 kHz, stored as float32."""
    cutoff = min(BASEBAND_CUTOFF_HZ / (sample_rate / 2), 0.99)
    return np.asarray(signal.firwin(BASEBAND_TAPS, cutoff, window="hamming"), dtype=np.float32)


def generate_mmse_taps() -> np.ndarray:
    """p25.py:1171-1192: (NSTEPS+1) x 8 raised-cosine-windowed sinc; every tap is formed in float64 and stored as
    float32, t == 0 gives 1.0, |t| >= 4 gives 0; each row is divided by its float32 sum when that sum is > 0."""
    taps = np.zeros((MMSE_NSTEPS + 1, MMSE_NTAPS), dtype=np.float32)
    for step in range(MMSE_NSTEPS + 1):
        mu = step / MMSE_NSTEPS
        for tap in range(MMSE_NTAPS):
            t = tap - 3 - mu
            if abs(t) < 1e-6:
                taps[step, tap] = 1.0
            else:
                sinc_val = np.sin(np.pi * t) / (np.pi * t)
                window = 0.5 * (1 + np.cos(np.pi * t / 4)) if abs(t) < 4 else 0
                taps[step, tap] = sinc_val * window
        s = np.sum(taps[step])
        if s > 0:
            taps[step] /= s
    return taps


def _state_dict(out) -> dict:
    d = {}
    for k, name in enumerate(STATE_VARS):
        d[name] = out[k]
        d[name + "_is_f32"] = bool(out[7 + k])
    d["last_phase"] = out[6]
    d["history_idx"] = int(out[13])
    d["symbol_count"] = int(out[14])
    d["history"] = np.array(out[15:23], dtype=np.float32)
    return d


class DiscriminatorBank(_lib.SymbolBank):
    """n_channels independent DiscriminatorDemodulators (one reference demodulate() call per channel and call)."""

    _prefix = "wh_disc_bank"
    _growth = 1.5

    def __init__(self, n_channels: int, sample_rate: int = 48000, symbol_rate: int = 4800,
                 max_samples_per_call: int = 1 << 14):
        self._torch = _lib.require_gpu()
        self.n_channels = int(n_channels)
        self.sample_rate, self.symbol_rate = sample_rate, symbol_rate
        self.samples_per_symbol = sample_rate / symbol_rate
        self.max_samples_per_call = int(max_samples_per_call)
        self._baseband_taps = np.ascontiguousarray(design_baseband_filter(sample_rate))
        self._mmse_taps = np.ascontiguousarray(generate_mmse_taps())
        self._create_bank(self.n_channels, float(sample_rate), float(symbol_rate), _lib.dptr(self._baseband_taps, "f32"),
                          len(self._baseband_taps), _lib.dptr(self._mmse_taps, "f32"), self.max_samples_per_call)

    def _size_outputs(self) -> None:
        self.cap = self.max_samples_per_call                 # at most one symbol per sample
        self._dibits = self._torch.empty((self.n_channels, self.cap), dtype=self._torch.uint8, device="cuda")

    def reset(self, channel: int = -1, full: bool = False) -> None:
        """full=False: DiscriminatorDemodulator.reset() (keeps the input gain); full=True: a fresh demodulator."""
        _lib.check(_lib.lib.wh_disc_bank_reset(self._h, int(channel), int(bool(full)), _lib.stream_ptr(self._torch)),
                   "wh_disc_bank_reset")

    def state(self, channel: int = 0) -> dict:
        """Loop values (float32 ones held exactly) with their "is float32" flags, the carried unwrapped phase, the MMSE
        history in the reference's ring layout, its index and the symbol count."""
        out = (C.c_double * 23)()
        _lib.check(_lib.lib.wh_disc_bank_get_state(self._h, int(channel), out, _lib.stream_ptr(self._torch)),
                   "wh_disc_bank_get_state")
        return _state_dict(out)

    @staticmethod
    def _mask(active, n):
        if active is None:
            return None
        act = np.ascontiguousarray(active, dtype=np.uint8)
        assert act.shape == (n,)
        return act

    def demodulate_device(self, audio_dev, active=None):
        """audio_dev float32 GPU tensor [C, n] (row stride >= n) -> (dibits uint8 [C, cap], counts int32 [C]), the
        bank's own buffers (valid until the next call).  Inactive channels and rows holding a non-finite sample keep
        their state and report 0 symbols."""
        torch = self._torch
        n, stride = self._call_shape(audio_dev, torch.float32)
        self._grow_for(n)
        act = self._mask(active, self.n_channels)
        _lib.check(_lib.lib.wh_disc_bank_run(self._h, audio_dev.data_ptr(), n, stride,
                                             None if act is None else act.ctypes.data, self._dibits.data_ptr(),
                                             self.cap, self._counts.data_ptr(), _lib.stream_ptr(torch)),
                   "wh_disc_bank_run")
        return self._dibits, self._counts

    def demodulate_iq_device(self, iq_dev, active=None, disc_out=None):
        """iq_dev complex64 GPU tensor [C, n] of decimated IQ -> discriminator (float64 angle, unwrap against the
        carried phase, diff) -> demodulator.  disc_out (optional) float32 [C, >= n] receives the disc audio."""
        torch = self._torch
        n, stride = self._call_shape(iq_dev, torch.complex64)
        self._grow_for(n)
        if disc_out is not None:
            assert disc_out.dtype == torch.float32 and disc_out.is_cuda and disc_out.shape[0] == self.n_channels
            assert disc_out.stride(1) == 1 and (self.n_channels == 1 or disc_out.stride(0) == stride)
            assert disc_out.shape[1] >= n
        act = self._mask(active, self.n_channels)
        _lib.check(_lib.lib.wh_disc_bank_run_iq(self._h, iq_dev.data_ptr(), n, stride,
                                                None if act is None else act.ctypes.data,
                                                None if disc_out is None else disc_out.data_ptr(),
                                                self._dibits.data_ptr(), self.cap, self._counts.data_ptr(),
                                                _lib.stream_ptr(torch)), "wh_disc_bank_run_iq")
        return self._dibits, self._counts

    def demodulate(self, audio, active=None) -> list:
        """audio float32 [C, n] host array = one reference call per channel -> list of dibit arrays (None for an
        inactive channel)."""
        x = np.ascontiguousarray(audio, dtype=np.float32)
        assert x.ndim == 2 and x.shape[0] == self.n_channels
        if x.shape[1] == 0:
            return [np.array([], dtype=np.uint8) if active is None or active[k] else None for k in range(self.n_channels)]
        d, cnt = self.demodulate_device(self._torch.from_numpy(x).cuda(), active)
        dib = self._to_host(cnt, d)[0]
        return [dib[k] if active is None or active[k] else None for k in range(self.n_channels)]


class DiscriminatorDemodulator:
    """Single-channel drop-in for decoders/p25.py:1105 (same ctor, attributes, demodulate / reset contract)."""

    BASEBAND_CUTOFF_HZ = BASEBAND_CUTOFF_HZ
    MMSE_NTAPS = MMSE_NTAPS
    MMSE_NSTEPS = MMSE_NSTEPS

    def __init__(self, sample_rate: int = 48000, symbol_rate: int = 4800) -> None:
        self.sample_rate = sample_rate
        self.symbol_rate = symbol_rate
        self.samples_per_symbol = sample_rate / symbol_rate
        self._bank = DiscriminatorBank(1, sample_rate, symbol_rate)
        self._baseband_taps = self._bank._baseband_taps
        self._mmse_taps = self._bank._mmse_taps

    def reset(self) -> None:
        self._bank.reset(0, full=False)

    def state(self) -> dict:
        return self._bank.state(0)

    def demodulate(self, audio) -> np.ndarray:
        audio = np.asarray(audio)
        if audio.size == 0:
            return np.array([], dtype=np.uint8)
        return self._bank.demodulate(audio.astype(np.float32, copy=False).reshape(1, -1))[0]


class VoiceRecorderBank:
    """The DSP of VoiceRecorder.process_iq for n_recorders recorders sharing one wideband buffer per call.

    Per call: the host-side gates of the reference -- an empty or non-finite wideband chunk leaves every state unchanged
    (system.py:527-541), |offset| > fs/2 - 50 kHz skips that recorder (:544-559) -- then TrunkingDDCBank (phase-continuous
    NCO + two-stage decimator) and the discriminator bank (angle / unwrap / diff with the carried unwrapped phase, then
    DiscriminatorDemodulator) in one launch sequence.  A decimated row holding a non-finite sample is dropped on the
    device with its state untouched (:658-669).

    The one host synchronisation is the finiteness check of the wideband chunk (a device reduction read back as one
    boolean): the reference drops a non-finite chunk before any state moves, and the DDC's filter state would
    otherwise advance on it."""

    MAX_RECORDERS = TrunkingDDCBank.MAX_CHANNELS

    def __init__(self, n_recorders: int, sample_rate: int, max_samples_per_call: int = 1 << 20):
        self._torch = _lib.require_gpu()
        self.n_recorders, self.sample_rate = int(n_recorders), int(sample_rate)
        self.max_samples_per_call = int(max_samples_per_call)
        self.ddc = TrunkingDDCBank(self.n_recorders, self.sample_rate, plan="recorder",
                                   max_samples_per_call=max_samples_per_call)
        self.output_rate = self.ddc.output_rate
        self.disc = DiscriminatorBank(self.n_recorders, 48000, 4800,
                                      max_samples_per_call=max(1, self.ddc.out_len(max_samples_per_call)))
        self.max_offset_hz = self.sample_rate / 2 - 50000
        self.offsets_hz = np.zeros(self.n_recorders, dtype=np.float64)
        self.assigned = np.zeros(self.n_recorders, dtype=bool)

    def assign(self, k: int, offset_hz: float) -> None:
        """Recorder k takes a new call at offset_hz: fresh front-end (filter state, NCO index) and a fresh slicer
        (VoiceRecorder.assign, system.py:386-393, + start_voice_channel's new P25Decoder, :446)."""
        self.ddc.reset(int(k))
        self.disc.reset(int(k), full=True)
        self.offsets_hz[k] = float(offset_hz)
        self.assigned[k] = True

    def release(self, k: int) -> None:
        """Recorder k goes idle: skipped by every call until it is assigned again."""
        self.assigned[k] = False

    def _run_mask(self, active) -> np.ndarray:
        act = self.assigned.copy()
        if active is not None:
            act &= np.asarray(active, dtype=bool)
        act &= np.abs(self.offsets_hz) <= self.max_offset_hz      # outside the capture band: skipped (:544-559)
        return act

    def process_device(self, iq_dev, offsets_hz=None, active=None):
        """iq_dev complex64 GPU tensor [n] -> (dibits uint8 [R, cap], counts int32 [R], disc_audio float32 [R, m]) on the
        device, or None when the chunk is empty or non-finite (nothing ran, no state moved).  offsets_hz (optional)
        updates the recorders' offsets; active (optional) masks recorders for this call.  Rows of skipped recorders
        (counts 0) are left as they were."""
        torch = self._torch
        assert iq_dev.is_cuda and iq_dev.dtype == torch.complex64 and iq_dev.is_contiguous()
        if offsets_hz is not None:
            offs = np.asarray(offsets_hz, dtype=np.float64)
            assert offs.shape == (self.n_recorders,)
            self.offsets_hz[:] = offs
        if iq_dev.numel() == 0:
            return None
        if not bool(torch.isfinite(torch.view_as_real(iq_dev)).all()):   # the one host synchronisation
            return None
        act = self._run_mask(active)
        if not act.any():
            return None
        n = iq_dev.numel()
        m = self.ddc.out_len(n)
        if n > self.max_samples_per_call:
            raise ValueError(f"VoiceRecorderBank: chunk of {n} samples exceeds max_samples_per_call "
                             f"{self.max_samples_per_call}")
        act_u8 = act.astype(np.uint8)
        dec = self.ddc.process_device(iq_dev, self.offsets_hz, act_u8)
        disc = torch.empty((self.n_recorders, m), dtype=torch.float32, device=iq_dev.device)
        dib, cnt = self.disc.demodulate_iq_device(dec, act_u8, disc)
        return dib, cnt, disc

    def process(self, iq, offsets_hz=None, active=None) -> list:
        """-> per recorder: (dibits uint8, disc_audio float32), or None for a recorder that was skipped (idle, outside
        the band, or an empty / non-finite chunk)."""
        x = np.ascontiguousarray(iq, dtype=np.complex64)
        if x.size == 0:
            if offsets_hz is not None:
                self.offsets_hz[:] = np.asarray(offsets_hz, dtype=np.float64)
            return [None] * self.n_recorders
        r = self.process_device(self._torch.from_numpy(x).cuda(), offsets_hz, active)
        if r is None:
            return [None] * self.n_recorders
        dib, cnt, disc = r
        act = self._run_mask(active)
        cnt = cnt.cpu().numpy()
        m = int(cnt.max()) if cnt.size else 0
        d = dib[:, :m].cpu().numpy()
        a = disc.cpu().numpy()
        out = []
        for k in range(self.n_recorders):
            if not act[k]:
                out.append(None)
            else:
                out.append((d[k, :cnt[k]].copy(), a[k].copy()))
        return out

    def state(self, k: int) -> dict:
        return self.disc.state(int(k))

