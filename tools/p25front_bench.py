#!/usr/bin/env python3
"""P25 channel front timing: 64 channels x one capture chunk (max(8192, fs // 20) samples, 50 ms) at 2.4 MS/s (resample
branch, 1/50, 1001 taps) and 6 MS/s (subsample branch, every 125th sample), device resident.  Prints one JSON line: per
rate the median over --iters calls (after --warmup) of the front alone (P25ChannelFront.process_device) and of front
plus LSM (P25ChannelBank.process_device, which includes its one host synchronisation, the finiteness check), in us,
timed with device events.

    python3 tools/p25front_bench.py [--channels 64] [--iters 20] [--warmup 5]
"""

from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "wavecap-sdr_amd")):
    sys.path.insert(0, p)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=64)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    import torch
    import signals as S
    import wavehip

    assert torch.cuda.is_available(), "p25front_bench needs a GPU"

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        us = []
        for _ in range(args.iters):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            us.append(a.elapsed_time(b) * 1e3)
        return float(np.median(us))

    out = {"channels": args.channels, "iters": args.iters, "device": torch.cuda.get_device_name(0)}
    for fs in (2_400_000, 6_000_000):
        n = max(8192, fs // 20)
        x = torch.from_numpy(S.noise_c64(n, 3)).cuda()
        offs = np.linspace(-0.4 * fs, 0.4 * fs, args.channels)
        front = wavehip.P25ChannelFront(args.channels, fs, max_samples_per_call=n)
        front.set_offsets(offs)
        bank = wavehip.P25ChannelBank(args.channels, fs, modulation="lsm", max_samples_per_call=n)
        bank.front.set_offsets(offs)
        out[f"front_us_{fs}"] = round(timed(lambda: front.process_device(x)), 1)
        out[f"front_lsm_us_{fs}"] = round(timed(lambda: bank.process_device(x)), 1)
        out[f"outputs_per_channel_{fs}"] = front.out_len(n)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
