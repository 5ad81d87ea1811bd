"""The field-staging rules of the twelve diagnostics, checked through every accumulator's ``add`` and every one-shot function.

Two tables.  The first feeds one bad argument at a time, in every position an entry point has (alone, as ``real``, as ``fake``),
with the library and the op backend patched to raise: the error must come from the argument checks and name the offending value.
The second runs five layouts through a recording op backend and looks at what reaches ``eof_fields`` and the kernel: the first
``n_valid`` fields, the caller's own storage wherever the batch is dense, a contiguous copy only where it is not.

Both tables hold on the commit before ``downgan_amd/fields.py`` existed, with one exception: the rows of
``test_two_devices_are_rejected`` for FractionsSkill, GridStats, GridHist, Temporal, Objects and Distances.  Those six took a
``fake`` series on another device than ``real`` without a word (only ValueJoint, Increments and the paired spectra checked it);
the shared pair check gave them the check."""
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from downgan_amd import _lib, backend, distmap, fss, gridhist, gridstats, histograms, increments, joint, objects, spectra, temporal

T = 2


def _no_library(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("library or device touched before the arguments were checked")
    monkeypatch.setattr(_lib, "lib", boom)
    monkeypatch.setattr(backend, "make_ops", boom)
    for m in (histograms, spectra, joint, increments):
        monkeypatch.setattr(m, "_ops", {})


# ---------------------------------------------------------------------------------------------------------- entry points
class Entry:
    """One accumulator and its one-shot functions.  style: how the layout flags are passed ("one": nhwc of the only series;
    "ab": nhwc / nhwc_b; "pair": nhwc as one flag or a pair).  grid: "fixed" (the accumulator is made for one), "pair" (the two
    series must agree) or None.  shots: the one-shot function without and with a second series; shot_n_valid: whether those take
    n_valid; has_spec: whether the channel count is fixed by a spec (else by the accumulator or the partner)."""

    def __init__(self, name, side, positions, style, grid, make, shots, shot_n_valid=True, has_spec=True):
        self.name, self.side, self.positions, self.style, self.grid = name, side, positions, style, grid
        self.make, self.shots, self.shot_n_valid, self.has_spec = make, shots, shot_n_valid, has_spec

    def flags(self, nhwc):
        if self.style == "one":
            return {"nhwc": nhwc[0]}
        if self.style == "ab":
            return {"nhwc": nhwc[0], "nhwc_b": nhwc[1]}
        return {"nhwc": nhwc}

    def add(self, real, fake, nhwc=(False, False), channels=None, n_valid=None, ops=None):
        acc = self.make(fake is not None, ops)
        series = (real,) if self.style == "one" else (real, fake)
        return acc.add(*series, n_valid=n_valid, channels=channels, **self.flags(nhwc))

    def shot(self, real, fake, nhwc=(False, False), channels=None, n_valid=None):
        kw = {"n_valid": n_valid} if self.shot_n_valid else {}
        flags = self.flags(nhwc)
        if fake is None and self.style == "ab":
            flags.pop("nhwc_b")
        return self.shots[fake is not None](real, fake, channels=channels, **flags, **kw)


HS = histograms.HistSpec.zscore(2, bins=64, lim=6.0)
JS_A = joint.JointSpec([(joint.Axis("a", 0, 8, -1.0, 1.0), joint.Axis("a", 1, 8, -1.0, 1.0))], 2, speed=None)
JS_AB = joint.JointSpec.zscore(2)
DEV = {"device": "cpu"}
ONE, PAIR, BOTH = ("alone",), ("real", "fake"), ("alone", "real", "fake")

ENTRIES = [
    Entry("histograms", 8, ONE, "one", None, lambda p, o: histograms.ValueHistogram(HS, ops=o, **DEV),
          {False: lambda a, b, **k: histograms.histogram(a, HS, **k)}, shot_n_valid=False),
    Entry("rapsd", 16, ONE, "one", "fixed", lambda p, o: spectra.RadialSpectrum(2, 16, ops=o, **DEV),
          {False: lambda a, b, **k: spectra.rapsd(a, **k)}, shot_n_valid=False, has_spec=False),
    Entry("cross", 16, PAIR, "ab", "pair", lambda p, o: spectra.CrossSpectrum(2, 16, ops=o, **DEV),
          {True: lambda a, b, **k: spectra.cross_rapsd(a, b, **k)}, shot_n_valid=False, has_spec=False),
    Entry("helmholtz", 16, BOTH, "ab", "pair", lambda p, o: spectra.HelmholtzSpectrum(16, ops=o, **DEV),
          {False: lambda a, b, **k: spectra.helmholtz_rapsd(a, **k), True: lambda a, b, **k: spectra.helmholtz_cross(a, b, **k)},
          shot_n_valid=False, has_spec=False),
    Entry("fss", 8, PAIR, "pair", "fixed", lambda p, o: fss.FractionsSkill(fss.FssSpec.zscore(2), 8, 8, ops=o, **DEV),
          {True: lambda a, b, **k: fss.fss(a, b, spec=fss.FssSpec.zscore(2), **k)}),
    Entry("gridstats", 8, BOTH, "pair", "fixed", lambda p, o: gridstats.GridStats(gridstats.GridSpec.zscore(2), 8, 8, paired=p, ops=o, **DEV),
          dict.fromkeys((False, True), lambda a, b, **k: gridstats.gridstats(a, b, spec=gridstats.GridSpec.zscore(2), **k))),
    Entry("gridhist", 8, BOTH, "pair", "fixed", lambda p, o: gridhist.GridHist(HS, 8, 8, paired=p, ops=o, **DEV),
          dict.fromkeys((False, True), lambda a, b, **k: gridhist.gridhist(a, b, spec=HS, **k))),
    Entry("joint", 8, BOTH, "pair", "pair", lambda p, o: joint.ValueJoint(JS_AB if p else JS_A, ops=o, **DEV),
          {False: lambda a, b, **k: joint.joint_histogram(a, JS_A, **k), True: lambda a, b, **k: joint.joint_histogram(a, JS_AB, b, **k)},
          shot_n_valid=False),
    Entry("increments", 8, BOTH, "pair", "pair", lambda p, o: increments.Increments(increments.IncrementSpec.zscore(2), ops=o, **DEV),
          dict.fromkeys((False, True), lambda a, b, **k: increments.increments(a, b, spec=increments.IncrementSpec.zscore(2), **k))),
    Entry("temporal", 8, BOTH, "pair", "fixed", lambda p, o: temporal.Temporal(temporal.TemporalSpec.zscore(2), 8, 8, paired=p, ops=o, **DEV),
          dict.fromkeys((False, True), lambda a, b, **k: temporal.temporal(a, b, spec=temporal.TemporalSpec.zscore(2), **k))),
    Entry("objects", 8, BOTH, "pair", "fixed", lambda p, o: objects.Objects(objects.ObjectSpec.zscore(2), 8, 8, paired=p, ops=o, **DEV),
          dict.fromkeys((False, True), lambda a, b, **k: objects.objects(a, b, spec=objects.ObjectSpec.zscore(2), **k))),
    Entry("distmap", 8, PAIR, "pair", "fixed", lambda p, o: distmap.Distances(distmap.DistSpec.zscore(2), 8, 8, ops=o, **DEV),
          {True: lambda a, b, **k: distmap.distances(a, b, spec=distmap.DistSpec.zscore(2), **k)}),
    Entry("distance_transform", 8, ONE, "one", None, None,
          {False: lambda a, b, **k: distmap.distance_transform(a, spec=distmap.DistSpec.zscore(2), **k)}, shot_n_valid=False),
]
IDS = [e.name for e in ENTRIES]


def _calls(e, pos, x, good, x_nhwc=False, **kw):
    """The calls of entry ``e`` with ``x`` in position ``pos`` (``good`` in the other): add, then the one-shot function."""
    real, fake = {"alone": (x, None), "real": (x, good), "fake": (good, x)}[pos]
    nhwc = kw.pop("nhwc", {"alone": (x_nhwc, x_nhwc), "real": (x_nhwc, False), "fake": (False, x_nhwc)}[pos])
    out = []
    if e.make is not None and not (fake is None and e.style == "ab"):  # the paired spectra have no one-sided accumulator
        out.append(("add", lambda: e.add(real, fake, nhwc=nhwc, **kw)))
    if (fake is not None) in e.shots and (e.shot_n_valid or "n_valid" not in kw):
        out.append(("shot", lambda: e.shot(real, fake, nhwc=nhwc, **kw)))
    return out


def _raises(e, pos, x, err, match, only=("add", "shot"), **kw):
    good = torch.zeros(T, 2, e.side, e.side)
    ran = 0
    for kind, call in _calls(e, pos, x, good, **kw):
        if kind in only:
            with pytest.raises(err, match=match):
                call()
            ran += 1
    return ran


# ------------------------------------------------------------------------------------------------ the table of bad inputs
@pytest.mark.parametrize("e", ENTRIES, ids=IDS)
def test_one_series_is_checked_in_every_position(monkeypatch, e):
    _no_library(monkeypatch)
    s = e.side
    rows = [
        (np.zeros((T, 2, s, s), np.float32), {}, TypeError, "ndarray"),
        (torch.zeros(T, 2, s, s, dtype=torch.float64), {}, TypeError, r"torch\.float64"),
        (torch.zeros(T, s, s), {}, ValueError, re.escape(str((T, s, s)))),
        (torch.zeros(0, 2, s, s), {}, ValueError, "at least one field"),
        (torch.zeros(T, s, s, 4), {"x_nhwc": True, "channels": 5}, ValueError, "channels = 5"),
        (torch.zeros(T, 9, s, s), {}, ValueError, "C = 9"),
    ]
    for pos in e.positions:
        for x, kw, err, match in rows:
            assert _raises(e, pos, x, err, match, **kw) >= 1


@pytest.mark.parametrize("e", ENTRIES, ids=IDS)
def test_a_series_agrees_with_its_owner_and_its_partner(monkeypatch, e):
    _no_library(monkeypatch)
    s = e.side
    for pos in e.positions:
        # three channels where the spec (the accumulator, the partner) has two
        x = torch.zeros(T, 3, s, s)
        if e.has_spec:
            assert _raises(e, pos, x, ValueError, r"C = 2 .*hold 3|differ in channels \((2 and 3|3 and 2)\)")
        elif e.name == "rapsd":
            assert _raises(e, pos, x, ValueError, r"RadialSpectrum.* 3\b", only=("add",))
        elif pos != "alone":
            assert _raises(e, pos, x, ValueError, r"paired.*\b3\b")
        # another grid than the accumulator's (one-shot: than the partner's)
        x, name = torch.zeros(T, 2, 2 * s, 2 * s), f"{2 * s} x {2 * s}|{re.escape(str((2 * s, 2 * s)))}"
        if e.grid == "fixed":
            assert _raises(e, pos, x, ValueError, name, only=("add", "shot") if pos == "fake" else ("add",))
        elif e.grid == "pair" and pos != "alone":
            assert _raises(e, pos, x, ValueError, rf"paired.*\b{2 * s}\b" if e.style == "ab" else name)
        # one field more than the partner
        if pos != "alone":
            x = torch.zeros(T + 1, 2, s, s)
            match = rf"paired.*\b{T + 1}\b" if e.style == "ab" else rf"differ in length \(({T} and {T + 1}|{T + 1} and {T})\)"
            assert _raises(e, pos, x, ValueError, match)


@pytest.mark.parametrize("e", [e for e in ENTRIES if e.style == "pair"], ids=[e.name for e in ENTRIES if e.style == "pair"])
def test_nhwc_is_one_flag_or_a_pair(monkeypatch, e):
    _no_library(monkeypatch)
    for pos in e.positions:
        assert _raises(e, pos, torch.zeros(T, 2, e.side, e.side), ValueError, r"nhwc.*\(True, False, True\)", nhwc=(True, False, True))


@pytest.mark.parametrize("e", ENTRIES, ids=IDS)
def test_n_valid_lies_in_the_batch(monkeypatch, e):
    _no_library(monkeypatch)
    ran = 0
    for pos in e.positions:
        for n in (0, T + 1, -1):
            ran += _raises(e, pos, torch.zeros(T, 2, e.side, e.side), ValueError, f"n_valid = {n} ", n_valid=n)
    assert ran >= 3 * (e.make is not None)


@pytest.mark.parametrize("e", [e for e in ENTRIES if "fake" in e.positions], ids=[e.name for e in ENTRIES if "fake" in e.positions])
def test_two_devices_are_rejected(monkeypatch, e):
    """NEW with downgan_amd/fields.py for fss, gridstats, gridhist, temporal, objects and distmap (see the module docstring);
    joint, increments and the paired spectra had the check before."""
    _no_library(monkeypatch)
    fake = torch.zeros(T, 2, e.side, e.side, device="meta")
    assert _raises(e, "fake", fake, ValueError, "meta", only=("add",)) == 1


# ------------------------------------------------------------------------------------------- what reaches the op backend
class Recorder:
    """An op backend that keeps what ``eof_fields`` was given and what each kernel method was called with, and computes
    nothing.  Every workspace size is one byte, so no caller splits a batch of this size."""

    device = torch.device("cpu")

    def __init__(self):
        self.described, self.kernels = [], []

    def eof_fields(self, x, nhwc=False, channels=None):
        self.described.append(SimpleNamespace(x=x, nhwc=nhwc, channels=channels))
        return self.described[-1]

    def __getattr__(self, name):
        if name.endswith("_ws_bytes"):
            return lambda *a, **k: 1

        def kernel(*a, **k):
            self.kernels.append((name, [v for v in a if isinstance(v, SimpleNamespace)]))
            if k.get("records") is not None:
                k["records"].zero_()
            if k.get("sum") is not None:
                k["sum"].zero_()
            if name == "objects":
                return torch.zeros(0, 12, dtype=torch.int64), None, 1
        return kernel


def _layouts(s, n=3):
    """(name, series, nhwc, channels, dense) of five layouts of n fields with two channels to read on an s x s grid."""
    g = torch.Generator().manual_seed(5)
    r = lambda *shape: torch.randn(*shape, generator=g)
    store = r(n, s, s, 4).to(torch.bfloat16)
    return [("nchw_fp32", r(n, 2, s, s), False, None, True),
            ("nhwc_bf16_padded", store, True, 2, True),
            ("nchw_more_channels", r(n, 4, s, s), False, 2, True),
            ("strided_view", r(n, 2, 2 * s, s)[:, :, ::2], False, None, False),
            ("native_batch", SimpleNamespace(nhwc=store.clone(), channels=2), False, None, True)]


@pytest.mark.parametrize("e", [e for e in ENTRIES if e.make is not None], ids=[e.name for e in ENTRIES if e.make is not None])
def test_descriptors_point_into_the_callers_storage(monkeypatch, e):
    _no_library(monkeypatch)
    n = 3
    for (name, xa, nhwc, channels, dense), (_, xb, _, _, _) in zip(_layouts(e.side, n), _layouts(e.side, n)):
        modes = ["alone"] * ("alone" in e.positions and e.style != "ab") + ["pair"] * ("fake" in e.positions)
        for pos in modes:
            o = Recorder()
            e.add(xa, None if pos == "alone" else xb, nhwc=(nhwc, nhwc), channels=channels, n_valid=n - 1, ops=o)
            assert len(o.kernels) == 1, (name, o.kernels)
            sent = o.kernels[0][1]
            assert len(sent) == (1 if pos == "alone" else 2), name
            for d, src in zip(sent, (xa, xb)):
                t = getattr(src, "nhwc", src)
                is_nhwc = nhwc or hasattr(src, "nhwc")
                assert d.x.shape[0] == n - 1, name
                if is_nhwc:
                    assert (d.nhwc, d.channels) == (True, 2) and d.x.shape[1:] == t.shape[1:], name
                else:
                    assert (d.nhwc, d.channels) == (False, None) and tuple(d.x.shape[1:]) == (2, e.side, e.side), name
                if dense:
                    assert d.x.data_ptr() == t.data_ptr() and d.x.dtype == t.dtype, name
                else:
                    assert d.x.is_contiguous() and d.x.data_ptr() != t.data_ptr() and torch.equal(d.x, t[:n - 1]), name
