"""GPU parity for the P25 channel front (wavehip.p25front): freq_shift -> decimate_iq_for_p25 (capture.py:166-295) against
the reference goldens of tools/gen_golden_p25front.py (outputs <= 1e-5 of peak, every rate branch, offset and call
length), the chained front -> LSMBank / C4FMBank path (dibits bit-exact, NID events equal to the reference framer's),
and the bank's own contracts (64-channel front == 64 one-channel fronts, active masking, non-finite chunks, growth,
reset)."""

import numpy as np
import pytest

import signals as S
from conftest import peak_rel_err

pytestmark = pytest.mark.gpu


def kept_index(m):
    """tools/gen_golden_p25front.py's stored output indices."""
    return np.unique(np.r_[np.arange(min(m, 96)), np.arange(max(0, m - 96), m), np.arange(0, m, 17)])


def _dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.complex64)).cuda()


def test_front_goldens_every_rate(golden):
    from wavehip import P25ChannelFront

    g = golden("p25front")
    for ri in range(int(g["n_rates"])):
        fs = int(g[f"r{ri}_fs"])
        offs = g[f"r{ri}_offsets"]
        front = P25ChannelFront(len(offs), fs, max_samples_per_call=max(8192, fs // 20))
        front.set_offsets(offs)
        for ci, n in enumerate(int(v) for v in g[f"r{ri}_lens"]):
            x = S.noise_c64(n, int(g[f"r{ri}_c{ci}_seed"]))
            out, rate = front.process_device(_dev(x))            # consecutive calls on one front
            assert rate == int(g[f"r{ri}_rate"])
            m = int(g[f"r{ri}_c{ci}_m"])
            assert out.shape == (len(offs), m), (fs, n)
            got = out.cpu().numpy()[:, kept_index(m)]
            want = g[f"r{ri}_c{ci}_out"]
            for k in range(len(offs)):
                assert peak_rel_err(got[k], want[k]) <= 1e-5, (fs, n, offs[k])


def test_decimate_iq_for_p25_drop_in(golden):
    from wavehip import decimate_iq_for_p25

    g = golden("p25front")
    for ri in range(int(g["n_rates"])):
        fs = int(g[f"r{ri}_fs"])
        n = int(g[f"r{ri}_lens"][0])
        x = S.noise_c64(n, int(g[f"r{ri}_c0_seed"]))
        y, rate = decimate_iq_for_p25(x, fs)                    # offset 0: freq_shift returns its input
        assert rate == int(g[f"r{ri}_rate"]) and y.dtype == np.complex64
        assert peak_rel_err(y[kept_index(len(y))], g[f"r{ri}_c0_out"][0]) <= 1e-5, fs
        if fs <= 48000:
            assert y is x
    e = np.zeros(0, dtype=np.complex64)
    assert decimate_iq_for_p25(e, 2_400_000)[0] is e


def _chain_input(mod, fs, seed, offset):
    n = 3 * max(8192, fs // 20)
    if mod == "lsm":
        return S.dqpsk_iq(n, fs, seed, symbol_rate=4800.0, snr_db=25.0, freq_offset_hz=offset + 40.0)[0]
    return S.c4fm_iq(n, fs, seed, snr_db=25.0, freq_offset_hz=offset + 40.0, dibits=S.nid_stream()[0])[0]


def test_chained_dibits_and_nid_events(golden):
    import wavehip

    g = golden("p25front_chain")
    lut = np.array([1.0, 3.0, -1.0, -3.0], dtype=np.float32)
    for ci in range(int(g["n_cases"])):
        mod, fs = str(g[f"k{ci}_mod"]), int(g[f"k{ci}_fs"])
        off = float(g[f"k{ci}_offset"])
        chunk = max(8192, fs // 20)
        x = _chain_input(mod, fs, int(g[f"k{ci}_seed"]), off)
        bank = wavehip.P25ChannelBank(1, fs, modulation=mod, max_samples_per_call=chunk)
        assert bank.p25_rate == int(g[f"k{ci}_rate"])
        fe = wavehip.P25NIDFrontEnd()
        events = []
        for k in range(3):
            (dib, soft), = bank.process(x[k * chunk:(k + 1) * chunk], offsets_hz=[off])
            assert np.array_equal(dib, g[f"k{ci}_dibits{k}"]), (mod, fs, k)
            if mod == "lsm":
                assert np.array_equal(soft, lut[dib]), (mod, fs, k)
            else:
                assert peak_rel_err(soft, g[f"k{ci}_soft{k}"]) <= 1e-5, (mod, fs, k)
            if len(dib):
                events += fe.process_batch(soft, dib)
        assert np.array_equal(np.array(events, dtype=np.int64).reshape(-1, 4), g[f"k{ci}_events"]), (mod, fs)
    assert int(g["seeds_kept"]) == int(g["n_cases"])


@pytest.mark.parametrize("fs", [2_400_000, 6_000_000, 200_000])
def test_64_channel_front_equals_64_single_fronts(fs):
    from wavehip import P25ChannelFront

    n = max(8192, fs // 20) + 5
    x = _dev(S.noise_c64(n, 77))
    offs = np.random.default_rng(5).uniform(-0.45 * fs, 0.45 * fs, 64).round(1)
    offs[:3] = (0.0, 12_500.5, -12_499.5)
    big, _ = P25ChannelFront(64, fs).process_device(x, offs)
    big = big.cpu().numpy()
    for k in range(64):
        one, _ = P25ChannelFront(1, fs).process_device(x, offs[k:k + 1])
        assert np.array_equal(big[k], one.cpu().numpy()[0]), k


def test_active_mask_leaves_rows_untouched():
    from wavehip import P25ChannelBank, P25ChannelFront

    fs = 2_400_000
    front = P25ChannelFront(5, fs)
    offs = np.array([0.0, 12_500.0, -25_000.0, 100_000.0, -7.0])
    a = _dev(S.noise_c64(fs // 20, 1))
    b = _dev(S.noise_c64(fs // 20, 2))
    first = front.process_device(a, offs)[0].cpu().numpy()
    act = np.array([1, 0, 1, 0, 0], dtype=bool)
    second = front.process_device(b, offs, active=act)[0].cpu().numpy()
    full = P25ChannelFront(5, fs).process_device(b, offs)[0].cpu().numpy()
    for k in range(5):
        assert np.array_equal(second[k], full[k] if act[k] else first[k]), k
    # the bank: inactive channels report nothing
    bank_out = P25ChannelBank(5, fs).process(S.noise_c64(fs // 20, 3), offs, active=act)
    assert [r is None for r in bank_out] == list(~act)


def test_non_finite_chunk_is_dropped():
    import wavehip

    fs, chunk, off = 2_400_000, 120_000, 312_500.0
    x = _chain_input("c4fm", fs, 11, off)
    bad = x[:chunk].copy()
    bad[777] = np.nan
    a = wavehip.P25ChannelBank(2, fs, modulation="c4fm")
    b = wavehip.P25ChannelBank(2, fs, modulation="c4fm")
    offs = [off, off - 12_500.0]
    assert a.process_device(_dev(bad), offs) is None
    assert a.process(bad, offs) == [None, None]
    for k in range(2):
        ra = a.process(x[k * chunk:(k + 1) * chunk], offs)
        rb = b.process(x[k * chunk:(k + 1) * chunk], offs)
        for (da, sa), (db, sb) in zip(ra, rb):
            assert np.array_equal(da, db) and np.array_equal(sa, sb)


def test_growth_beyond_max_samples_per_call():
    import wavehip
    from wavehip import P25ChannelFront

    for fs in (2_400_000, 8_000_000):
        n = fs // 20
        x = _dev(S.noise_c64(n, 21))
        offs = np.array([25_000.0, -50_000.0])
        small = P25ChannelFront(2, fs, max_samples_per_call=1000)
        ref = P25ChannelFront(2, fs, max_samples_per_call=n)
        got, _ = small.process_device(x, offs)
        assert small.max_samples_per_call >= n
        assert np.array_equal(got.cpu().numpy(), ref.process_device(x, offs)[0].cpu().numpy())
    fs, off = 2_400_000, 312_500.0
    xs = _chain_input("lsm", fs, 7300, off)
    grown = wavehip.P25ChannelBank(1, fs, max_samples_per_call=5000)
    sized = wavehip.P25ChannelBank(1, fs, max_samples_per_call=120_000)
    for k in range(2):
        ca = grown.process(xs[k * 120_000:(k + 1) * 120_000], [off])[0]
        cb = sized.process(xs[k * 120_000:(k + 1) * 120_000], [off])[0]
        assert np.array_equal(ca[0], cb[0]), k


def test_reset():
    import wavehip

    fs, chunk, off = 6_000_000, 300_000, 312_500.0
    x = _chain_input("lsm", fs, 7350, off)
    bank = wavehip.P25ChannelBank(1, fs)
    first = [bank.process(x[k * chunk:(k + 1) * chunk], [off])[0][0] for k in range(2)]
    bank.reset()
    again = [bank.process(x[k * chunk:(k + 1) * chunk], [off])[0][0] for k in range(2)]
    for a, b in zip(first, again):
        assert np.array_equal(a, b)
    with pytest.raises(ValueError):
        bank.reset(0)
