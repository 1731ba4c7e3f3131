"""Boundary facts of the drop-in against the reference package, from tests/golden/boundary_facts.json: the reference's
side of each fact (ChannelConfig fields and defaults, the FFT base surface, constructor / method signatures), recorded by
oracle/check_boundary.py --record, which also checks them and the registry / Capture-binding facts against the live
reference package."""

import dataclasses
import inspect
import json
import os
import subprocess
from types import SimpleNamespace

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def facts():
    with open(os.path.join(ROOT, "tests", "golden", "boundary_facts.json")) as fh:
        return json.load(fh)


def _params(f, skip_self=True):
    """[name, repr(default) or "<required>", kind] per parameter, as oracle/check_boundary.py records them."""
    p = [q for q in inspect.signature(f).parameters.values() if not q.name.startswith("_")]
    if skip_self and p and p[0].name == "self":
        p = p[1:]
    return [[q.name, "<required>" if q.default is inspect._empty else repr(q.default), q.kind.name] for q in p]


def _attr(obj, path):
    for part in path.split("."):
        obj = getattr(obj, part)
    return obj


def test_boundary_facts_against_the_reference(facts):
    import wavehip
    from wavehip import capture_seam, channel_ops, fft_backend

    fails = []

    def check(ok, what):
        if not ok:
            fails.append(what)

    # 1. ChannelConfig: every field of the reference's (id / capture_id aside) with the same defaults
    rf = {k: v for k, v in facts["channel_config"].items() if k not in ("id", "capture_id")}
    of = {f.name: f for f in dataclasses.fields(wavehip.ChannelConfig)}
    missing = [k for k in rf if k not in of]
    check(not missing, f"wavehip.ChannelConfig lacks reference fields {missing}")
    diff = [k for k in rf if k in of and "default" in rf[k] and not rf[k].get("factory")
            and of[k].default is not dataclasses.MISSING and of[k].default != rf[k]["default"]]
    check(not diff, f"ChannelConfig defaults differ from the reference's: {diff}")
    # ... and an object carrying exactly the reference ChannelConfig's fields at its defaults drives the chain builder
    ref_defaults = {k: v["default"] for k, v in facts["channel_config"].items() if "default" in v}
    for mode in ("nbfm", "wbfm", "am", "sam", "ssb", "raw", "p25", "dmr", "nxdn", "dstar", "ysf"):
        cfg = SimpleNamespace(**dict(ref_defaults, id="c1", capture_id="cap1", mode=mode, offset_hz=12500.0))
        try:
            if mode in ("raw", "p25", "dmr", "nxdn", "dstar", "ysf"):
                channel_ops._unsupported(cfg)
                channel_ops._chain_key(cfg)
            else:
                demod = channel_ops.build_chain(cfg, 48000)[0]
                check(demod in (0, 1, 2, 3, 4, 5), f"mode {mode!r}: build_chain gave demod {demod!r}")
        except Exception as e:  # noqa: BLE001
            check(False, f"reference ChannelConfig(mode={mode!r}): {type(e).__name__}: {e}")
    check(_params(wavehip.process_channel_dsp_stateless, False) == facts["process_channel_dsp_stateless"],
          "process_channel_dsp_stateless parameter list differs from the reference's")

    # 2. the FFT backend's base surface (the standalone mirror when the reference is not importable)
    check([f.name for f in dataclasses.fields(fft_backend.FFTResult)] == facts["fft_result_fields"], "FFTResult fields")
    check(sorted(fft_backend.FFTBackend.__abstractmethods__) == facts["fft_backend_abstract"], "FFTBackend abstract methods")
    check(_params(fft_backend.FFTBackend.__init__) == facts["fft_backend_init"], "FFTBackend.__init__ signature")
    check(_params(fft_backend.FFTBackend.execute) == facts["fft_backend_execute"], "FFTBackend.execute signature")
    check(issubclass(fft_backend.HipFFTBackend, fft_backend.FFTBackend) and not fft_backend.HipFFTBackend.__abstractmethods__,
          "HipFFTBackend implements the whole FFTBackend surface")
    check(_params(fft_backend.HipFFTBackend.execute) == facts["fft_backend_execute"], "HipFFTBackend.execute signature")

    # 3. without a GPU, construction raises ImportError (what the reference registry falls through on)
    if not fft_backend.is_available():
        try:
            fft_backend.HipFFTBackend(1024)
            check(False, "HipFFTBackend(1024) without a GPU did not raise")
        except ImportError:
            pass

    # 4. signatures: names, order and defaults agree; extra keyword-only / **kwargs tails are the drop-in's own business
    for rec in facts["signatures"]:
        pa, pb = rec["reference"], _params(_attr(wavehip, rec["wavehip"]))
        named = [x[0] for x in pa if x[2] != "VAR_KEYWORD"]
        same = [x[:2] for x in pa] == [x[:2] for x in pb[:len(pa)]] or \
            named == [x[0] for x in pb if x[2] != "VAR_KEYWORD"][:len(named)]
        check(same, f"{rec['name']} signature: reference {[x[:2] for x in pa]} vs wavehip {[x[:2] for x in pb]}")

    # 5. the batched seam takes Capture._process_channels_parallel's parameters after self
    check(facts["capture_process_channels_parallel"] == _params(capture_seam.process_channels_parallel)[1:],
          "process_channels_parallel parameters differ from Capture._process_channels_parallel's")

    assert not fails, "\n".join(fails)


def test_release_library_reads_no_environment_variables():
    """Tuning / diagnostic switches are explicit API calls (wh_pfb_tune, ChannelBank(iir_form=...)); the shipped library
    must not import getenv at all (a `make DIAG=1` measurement build does)."""
    so = os.path.join(ROOT, "wavecap-sdr_amd", "wavehip", "libwavehip.so")
    out = subprocess.run(["nm", "-D", "--undefined-only", so], capture_output=True, text=True).stdout
    assert "getenv" not in out, "libwavehip.so imports getenv: build it without DIAG=1"
