"""Row A12 (LSM): pin oracle/lsm_ref.c to the goldens captured from the reference's
decoders/p25.py CQPSKDemodulator (oracle/gen_golden.py lsm)."""

import numpy as np
import pytest

import signals as S
from oracle import lsm_c


def lsm_case(g, ci):
    fs, sr, n, seed, snr, off = g[f"c{ci}_args"]
    fs, sr, n, seed = int(fs), int(sr), int(n), int(seed)
    sps_i = int(round(fs / sr))
    x, _ = S.dqpsk_iq(n, sps_i * sr, seed, symbol_rate=sr, snr_db=float(snr), freq_offset_hz=float(off))
    if str(g[f"c{ci}_special"]) == "silence":
        x = x.copy()
        x[8000:9500] = 0
    assert S.sha256(x) == str(g[f"c{ci}_sha"])
    return fs, sr, x, [int(v) for v in g[f"c{ci}_lens"]]


def lsm_big_case(g, ci):
    """Input and call lengths of lsm_big case ci (oracle/gen_golden.py gen_lsm_big / lsm_big_input)."""
    fs, sr, seed, snr, off = g[f"c{ci}_args"]
    fs, sr, seed = int(fs), int(sr), int(seed)
    calls = [int(v) for v in g[f"c{ci}_calls"]]
    sps_i = int(round(fs / sr))
    x, _ = S.dqpsk_iq(sum(calls), sps_i * sr, seed, symbol_rate=sr, snr_db=float(snr), freq_offset_hz=float(off))
    lo, hi = (int(v) for v in g[f"c{ci}_muted"])
    if lo >= 0:
        x = x.copy()
        x[lo:hi] = 0
    assert S.sha256(x) == str(g[f"c{ci}_sha"])
    return fs, sr, x, calls


def check_lsm_against_golden(g, ci, dib, ph, cnt, st, f32mode):
    """The assertions of test_lsm_oracle_matches_reference for one case: counts and dibits bit-exact, phases within 2e-6
    rad over the first 500 symbols and 1e-2 after, end-of-call state within 2e-3."""
    assert np.array_equal(np.array(cnt), g[f"c{ci}_counts"]), f"case {ci}: symbol counts"
    assert np.array_equal(np.concatenate(dib), g[f"c{ci}_dibits"]), f"case {ci}: dibits"
    dphi = np.abs(np.concatenate(ph).astype(np.float64) - g[f"c{ci}_phases"])
    dphi = np.minimum(dphi, 2 * np.pi - dphi)
    assert dphi[:500].max() <= 2e-6 and dphi.max() <= 1e-2, f"case {ci}: phase {dphi[:500].max()} {dphi.max()}"
    st = np.array(st)
    ref = g[f"c{ci}_state"]
    wrap = np.abs(st[:, 2] - ref[:, 2])
    st[:, 2] = np.where(wrap > np.pi, ref[:, 2], st[:, 2])   # +-pi wrap of the NCO phase
    assert np.abs(st - ref).max() <= 2e-3, f"case {ci}: state"
    assert f32mode == bool(g[f"c{ci}_clock_is_f32"])


def test_lsm_designs_match_reference(golden):
    g = golden("lsm")
    assert np.array_equal(lsm_c.mmse_table(), g["mmse"])
    for ci in range(int(g["n_cases"])):
        fs = int(g[f"c{ci}_args"][0])
        assert np.array_equal(lsm_c.baseband_taps(fs), g[f"c{ci}_lpf"])


@pytest.mark.parametrize("flavour", [0, 1])
def test_lsm_oracle_matches_reference(golden, flavour):
    """Dibits and per-call symbol counts bit-exact for both math flavours.  Per-symbol phases: within 2e-6 rad
    over the first 500 symbols (pins the dtype semantics), within 1e-2 afterwards -- the reference's clock
    loop slips and a 1-ulp difference (SVML vs libm atan2f, BLAS order) occasionally moves the interpolator by
    one 1/128 step (see gen_golden.gen_lsm); end-of-call state within 2e-3."""
    g = golden("lsm")
    for ci in range(int(g["n_cases"])):
        fs, sr, x, lens = lsm_case(g, ci)
        r = lsm_c.LSMDemodulatorRef(fs, sr, flavour)
        pos, dib, ph, cnt, st = 0, [], [], [], []
        for ln in lens:
            o = r.demodulate(x[pos:pos + ln])
            pos += ln
            dib.append(o)
            ph.append(r.last_phases)
            cnt.append(len(o))
            s = r.state()
            st.append([s["agc_gain"], s["freq_offset"], s["phase_acc"], s["symbol_clock"],
                       s["prev_symbol"].real, s["prev_symbol"].imag])
        assert np.array_equal(np.array(cnt), g[f"c{ci}_counts"]), f"case {ci}: symbol counts"
        assert np.array_equal(np.concatenate(dib), g[f"c{ci}_dibits"]), f"case {ci}: dibits"
        dphi = np.abs(np.concatenate(ph).astype(np.float64) - g[f"c{ci}_phases"])
        dphi = np.minimum(dphi, 2 * np.pi - dphi)
        assert dphi[:500].max() <= 2e-6 and dphi.max() <= 1e-2, f"case {ci}: phase {dphi[:500].max()} {dphi.max()}"
        st = np.array(st)
        ref = g[f"c{ci}_state"]
        wrap = np.abs(st[:, 2] - ref[:, 2])
        st[:, 2] = np.where(wrap > np.pi, ref[:, 2], st[:, 2])   # +-pi wrap of the NCO phase
        assert np.abs(st - ref).max() <= 2e-3, f"case {ci}: state"
        assert r.state()["f32mode"] == bool(g[f"c{ci}_clock_is_f32"])


@pytest.mark.parametrize("flavour", [0, 1])
def test_lsm_oracle_matches_reference_at_monitor_call_sizes(golden, flavour):
    """lsm_big: whole 72 000 / 75 000-sample calls at 48 kHz (the monitor's buffer, trunking/system.py:1547-1548),
    37 500-sample calls at 25 kHz, a muted stretch and a weak signal inside one call -- the same assertions as above."""
    g = golden("lsm_big")
    assert int(g["n_cases"]) >= 1 and len(g["seeds_kept"]) == int(g["n_cases"])
    for ci in range(int(g["n_cases"])):
        fs, sr, x, calls = lsm_big_case(g, ci)
        assert max(calls) >= 37500
        r = lsm_c.LSMDemodulatorRef(fs, sr, flavour)
        pos, dib, ph, cnt, st = 0, [], [], [], []
        for ln in calls:
            o = r.demodulate(x[pos:pos + ln])
            pos += ln
            dib.append(o)
            ph.append(r.last_phases)
            cnt.append(len(o))
            s = r.state()
            st.append([s["agc_gain"], s["freq_offset"], s["phase_acc"], s["symbol_clock"],
                       s["prev_symbol"].real, s["prev_symbol"].imag])
        check_lsm_against_golden(g, ci, dib, ph, cnt, st, r.state()["f32mode"])
