#!/usr/bin/env python3
"""Voice-recorder pool timing: R recorders x one 100 ms chunk of 6 MS/s IQ through VoiceRecorderBank.process_device,
device resident.  Prints one JSON line: the median per call (after warm-up) of the DDC part (TrunkingDDCBank), the
slicer part (discriminator + DiscriminatorDemodulator bank), the whole process_device call (including its one host
synchronisation, the finiteness check), and the real-time factor per recorder.

    python3 tools/voice_bench.py [--recorders 64] [--iters 50] [--warmup 10]
    python3 tools/voice_bench.py --reference-cpu <reference backend dir>   # the reference's process_iq, one recorder,
                                                                            # on the CPU (build machine only)
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "wavecap-sdr_amd")):
    sys.path.insert(0, p)

FS, CHUNK = 6_000_000, 600_000      # 100 ms


def chunk_iq(seed: int = 3) -> np.ndarray:
    import signals as S
    return S.c4fm_iq(CHUNK, FS, seed, snr_db=20.0, freq_offset_hz=412_500.0)[0]


def gpu(args) -> dict:
    import torch
    import wavehip

    R = args.recorders
    x = torch.from_numpy(chunk_iq()).cuda()
    offs = np.linspace(-2_800_000.0, 2_800_000.0, R)
    bank = wavehip.VoiceRecorderBank(R, FS, max_samples_per_call=CHUNK)
    for k in range(R):
        bank.assign(k, offs[k])
    act = np.ones(R, dtype=np.uint8)
    m = bank.ddc.out_len(CHUNK)
    disc = torch.empty((R, m), dtype=torch.float32, device="cuda")

    def timed(fn, iters):
        ms = []
        for _ in range(iters):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        return float(np.median(ms))

    dec = bank.ddc.process_device(x, offs, act)
    parts = {
        "ddc": lambda: bank.ddc.process_device(x, offs, act),
        "slicer": lambda: bank.disc.demodulate_iq_device(dec, act, disc),
        "total": lambda: bank.process_device(x),
    }
    for fn in parts.values():
        timed(fn, args.warmup)
    res = {k: timed(fn, args.iters) for k, fn in parts.items()}
    _, cnt, _ = bank.process_device(x)
    torch.cuda.synchronize()
    return dict(recorders=R, chunk_ms=1e3 * CHUNK / FS, ddc_ms=res["ddc"], slicer_ms=res["slicer"],
                total_ms=res["total"], realtime_factor=res["total"] / (1e3 * CHUNK / FS),
                symbols_per_recorder=int(cnt.cpu().numpy().mean()), device=torch.cuda.get_device_name(0))


def reference_cpu(path: str, iters: int) -> dict:
    import logging
    sys.path.insert(0, path)
    logging.disable(logging.CRITICAL)
    import wavecapsdr.trunking  # noqa: F401
    from wavecapsdr.decoders import p25 as rp25
    from wavecapsdr.trunking import system as rsys

    r = rsys.VoiceRecorder(id="r0", system_id="s")
    r.setup_decimation_filter(FS, 48000)
    r.state = "recording"
    r._voice_channel = object()
    r.offset_hz = 412_500.0
    r._p25_decoder = rp25.P25Decoder(sample_rate=48000)
    x = chunk_iq()
    ts = []
    for i in range(iters + 2):
        t0 = time.perf_counter()
        try:
            r.process_iq(x, FS)
        except Exception:      # the vocoder hand-off after the demodulator needs an event loop
            pass
        if i >= 2:
            ts.append(time.perf_counter() - t0)
    return dict(reference_process_iq_ms=1e3 * float(np.median(ts)), recorders=1, chunk_ms=1e3 * CHUNK / FS)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--recorders", type=int, default=64)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reference-cpu", default=None)
    args = ap.parse_args()
    out = reference_cpu(args.reference_cpu, 5) if args.reference_cpu else gpu(args)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
