"""Temporal diagnostics without a GPU: the host reference dg_temporal_host against an independent numpy restatement (a Python loop
over t with np.float32 arithmetic), hand-made series with known answers, the chunking contract on the host, the host-side
derivations of ``TemporalResult``, spec and argument checks that fire before any library call, the ABI surface, and the trainer's
opt-in hook on the emulated ops (a test-local op class adds a numpy ``temporal`` under the usual make_ops patch)."""
import ctypes as C
import json
import os
import re
import subprocess
import types

import numpy as np
import pytest
import torch

from downgan_amd import _lib, histograms, temporal
from downgan_amd.temporal import ARRAYS, Temporal, TemporalResult, TemporalSpec

from .test_gridstats_cpu import _no_library
from .test_histograms_cpu import F32, bins_ref, transform_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FMAX = np.finfo(F32).max


# ------------------------------------------------------------------------------------------------- the definition in numpy
def specs():
    """with speed: 4 thresholds of both senses, 4 lags up to 24, 8 durations; one channel: one threshold, no lag, one duration
    row; no threshold: one lag, one bin; three channels, a speed of (2, 0), one "below" threshold, 4 lags, 512 bins."""
    return [("speed_4thr_4lag", TemporalSpec(2, scale=[2.0, 0.5], offset=[-1.0, 0.25], speed=(0, 1),
                                             thresholds=[[1.0, 2.0, -1.0, -3.0], [0.5, 1.0, 0.0, -0.5], [1.5, 2.5, 0.5, 0.25]],
                                             below=(False, False, True, True), ndur=8, lags=(1, 2, 3, 24), nbins=16, ranges=4.0)),
            ("one_thr_no_lag", TemporalSpec(1, speed=None, thresholds=[0.25], below=False, ndur=1, lags=())),
            ("no_thr_one_lag", TemporalSpec(2, speed=None, thresholds=(), lags=(1,), nbins=1, ranges=[[1.0], [0.5]])),
            ("below_512", TemporalSpec(3, speed=(2, 0), thresholds=[-0.5], below=True, ndur=1, lags=(2, 5, 7, 11), nbins=512,
                                       ranges=[1.0, 2.0, 3.0, 4.0]))]


def y_ref(spec, x):
    """x float32 [T, C, P] -> the output values float32 [T, nout, P] (test_histograms_cpu.transform_ref)."""
    T, Cn, P = x.shape
    y = transform_ref(spec, np.ascontiguousarray(x.transpose(1, 0, 2)).reshape(Cn, -1))
    return np.ascontiguousarray(y.reshape(spec.nout, T, P).transpose(1, 0, 2))


def ramp_rows(spec, j, l, d):
    """The rows of the ramps d (float32 [n]) of output channel j at lag index l: bins_ref on a one-channel identity spec."""
    one = types.SimpleNamespace(nout=1, bins=spec.nbins, speed=None, scale=np.ones(1, F32), offset=np.zeros(1, F32),
                                lo=spec.lo[j, l:l + 1], inv_w=spec.inv_w[j, l:l + 1])
    return bins_ref(one, d[None])[0]


def zero_state(spec, P):
    return {k: np.zeros(shape[1:], dtype=dt) for k, (shape, dt) in spec.shapes(1, P).items()}


def temporal_ref(spec, x, t0=0, state=None):
    """The seven arrays of one series after adding x (float32 [T, C, P]) as the times t0 .. : a Python loop over t, every fp32
    operation in np.float32, every sum in np.float64 in t order, vectorised over the pixels only."""
    T, _, P = x.shape
    st = zero_state(spec, P) if state is None else state
    R, nout = spec.R, spec.nout
    past = np.zeros((R + T, nout, P), dtype=F32)
    for ta in range(max(t0 - R, 0), t0):
        past[ta - (t0 - R)] = st["tail"][:, ta % R]
    past[R:] = y_ref(spec, x)
    with np.errstate(all="ignore"):
        for t in range(T):
            yt = past[R + t]
            for k in range(spec.nthr):
                thr = spec.thresholds[:, k][:, None]
                cond = (yt < thr) if spec.below[k] else (yt > thr)
                run = st["open"][:, k]
                ended = ~cond & (run > 0)
                for j in range(nout):
                    np.add.at(st["spells"][j, k], np.minimum(run[j][ended[j]], spec.ndur) - 1, 1)
                st["spellmap"][:, k, 0] += ended
                st["spellmap"][:, k, 1] += np.where(ended, run, 0)
                run[...] = np.where(cond, run + 1, 0)
                st["spellmap"][:, k, 2] = np.maximum(st["spellmap"][:, k, 2], run)
            fin, yd = np.isfinite(yt), yt.astype(np.float64)
            st["accnt"][:, 0] += fin
            st["acsum"][:, 0] = np.where(fin, st["acsum"][:, 0] + yd, st["acsum"][:, 0])
            st["acsum"][:, 1] = np.where(fin, st["acsum"][:, 1] + yd * yd, st["acsum"][:, 1])
            for l, tau in enumerate(spec.lags):
                if t0 + t - tau < 0:
                    continue
                yl = past[R + t - tau]
                d = (yt - yl).astype(F32)
                for j in range(nout):
                    np.add.at(st["ramps"][j, l], ramp_rows(spec, j, l, d[j]), 1)
                both, yld = fin & np.isfinite(yl), yl.astype(np.float64)
                st["accnt"][:, 1 + l] += both
                st["acsum"][:, 2 + 2 * l] = np.where(both, st["acsum"][:, 2 + 2 * l] + yd * yld, st["acsum"][:, 2 + 2 * l])
                st["acsum"][:, 3 + 2 * l] = np.where(both, st["acsum"][:, 3 + 2 * l] + (yd + yld), st["acsum"][:, 3 + 2 * l])
        for t in range(max(T - R, 0), T):
            st["tail"][:, (t0 + t) % R] = past[R + t]
    return st


def special_values(spec, c):
    """float32 inputs of channel c that land on every threshold of output channel c and on its two fp32 neighbours, +-0,
    denormals, +-inf, NaN and +-FLT_MAX."""
    vals = []
    for k in range(spec.nthr):
        on = F32((float(spec.thresholds[c, k]) - float(spec.offset[c])) / float(spec.scale[c]))
        vals += [on, np.nextafter(on, F32(-np.inf)), np.nextafter(on, F32(np.inf))]
    vals += [0.0, -0.0, 1e-45, -1e-45, 3e-39, -3e-39, np.inf, -np.inf, np.nan, FMAX, -FMAX]
    return np.array(vals, dtype=F32)


def data(rng, spec, T, P, cuts=()):
    """float32 [T, C, P]: an AR(1) process in t per pixel (so that spells last), the special values planted at known (t, p), a
    pixel that is never finite in channel 0, and around every chunk boundary of ``cuts`` a pixel that stays above every
    "above" threshold and one that stays below every "below" threshold, so that spells cross the boundary."""
    Cn = spec.C
    x = np.empty((T, Cn, P), dtype=F32)
    x[0] = rng.standard_normal((Cn, P))
    for t in range(1, T):
        x[t] = 0.8 * x[t - 1] + 0.6 * rng.standard_normal((Cn, P)).astype(F32)
    x *= 1.5
    for c in range(Cn):
        sv = special_values(spec, c)
        pos = (np.arange(len(sv)) * 7 + 3 + c) % (T * P)
        x[pos // P, c, pos % P] = sv
    if P > 20:
        x[:, 0, P - 1] = np.nan
    if P > 4:
        for cut in cuts:
            lo, hi = max(cut - 2, 0), min(cut + 2, T)
            x[lo:hi, :, 1] = 50.0                                    # y far above every threshold (scales are positive)
            x[lo:hi, :, 2] = -50.0
    return x


def same_bits(a, b, what=""):
    """Exact equality of two array dicts, NaN payloads and signed zeros included."""
    assert set(a) == set(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, (what, k, a[k].dtype, b[k].dtype, a[k].shape, b[k].shape)
        u = {4: np.uint32, 8: np.uint64}[a[k].dtype.itemsize]
        np.testing.assert_array_equal(np.ascontiguousarray(a[k]).view(u), np.ascontiguousarray(b[k]).view(u), err_msg=f"{what} {k}")


def host_chunks(spec, x, cuts):
    """The host reference fed the series cut at ``cuts``."""
    st, t0 = None, 0
    for part in np.split(x, list(cuts)):
        if len(part):
            st = temporal.host_temporal(spec, part, t0, st)
            t0 += len(part)
    return st


# ------------------------------------------------------------------------------------------------- the host reference
@pytest.mark.parametrize("shape", [(1, 1), (50, 1), (30, 35)])
@pytest.mark.parametrize("name,spec", specs())
def test_host_reference_against_numpy(name, spec, shape):
    T, P = shape
    x = data(np.random.default_rng(5), spec, T, P, cuts=(7,))
    got = temporal.host_temporal(spec, x)
    same_bits(got, temporal_ref(spec, x), f"{name} {shape}")
    if T > 8:                                                        # a second call continues the first: state, t0
        a = temporal.host_temporal(spec, x[:7])
        same_bits(a, temporal_ref(spec, x[:7]), f"{name} {shape} first part")
        b = temporal.host_temporal(spec, x[7:], 7, a)
        same_bits(b, temporal_ref(spec, x[7:], 7, temporal_ref(spec, x[:7])), f"{name} {shape} second part")
        same_bits(b, got, f"{name} {shape} two calls")
    if spec.nlag:
        assert got["ramps"].sum() == sum(max(T - tau, 0) for tau in spec.lags) * spec.nout * P
    if spec.nthr:
        assert (got["spellmap"][:, :, 1].sum(axis=-1) >= got["spells"].sum(axis=-1)).all()


@pytest.mark.parametrize("name,spec", specs())
def test_host_reference_does_not_depend_on_the_chunking(name, spec):
    T, P = 30, 35
    x = data(np.random.default_rng(6), spec, T, P, cuts=(2, 7, 15))
    one = host_chunks(spec, x, ())
    same_bits(host_chunks(spec, x, range(1, T)), one, f"{name} chunks of 1")
    same_bits(host_chunks(spec, x, (2, 7)), one, f"{name} chunks (2, 5, rest)")


def test_ramp_histograms_are_the_bins_of_the_numpy_differences():
    name, spec = specs()[0]
    T, P = 40, 9
    x = data(np.random.default_rng(8), spec, T, P)
    y = y_ref(spec, x)
    got = temporal.host_temporal(spec, x)["ramps"]
    with np.errstate(all="ignore"):
        for j in range(spec.nout):
            for l, tau in enumerate(spec.lags):
                d = (y[tau:, j] - y[:-tau, j]).astype(F32).reshape(-1)
                np.testing.assert_array_equal(got[j, l], np.bincount(ramp_rows(spec, j, l, d), minlength=spec.nbins + 3))
    assert got[:, :, -1].sum() > 0                                   # NaN and inf - inf were planted


# ------------------------------------------------------------------------------------------------- hand-made series
def hand_spec(**kw):
    return TemporalSpec(1, speed=None, **dict(dict(thresholds=[1.0], below=False, ndur=4, lags=(1, 20), nbins=8, ranges=4.0), **kw))


HAND = np.array([2, 2, 1, 2, 2, 2, 2, 2, np.nan, 2, 0, 2, 2], dtype=F32)


@pytest.mark.parametrize("cuts", [(), (4,), tuple(range(1, 13))])
def test_hand_made_spells(cuts):
    """y > 1: times 0-1 (ended by a value EQUAL to the threshold), 3-7 (length 5 >= ndur = 4: the last row; it straddles the
    chunk boundary at 4; ended by NaN), 9 (length 1), and 11-12, still open at the end: censored, not a spell."""
    spec = hand_spec()
    st = host_chunks(spec, HAND.reshape(-1, 1, 1), cuts)
    np.testing.assert_array_equal(st["spells"][0, 0], [1, 1, 0, 1])
    np.testing.assert_array_equal(st["spellmap"][0, 0, :, 0], [3, 8, 5])
    np.testing.assert_array_equal(st["open"][0, 0], [2])
    res = TemporalResult.from_state(spec, 1, 1, len(HAND), st)
    np.testing.assert_array_equal(res.spell_counts()[0, 0], [1, 1, 0, 1])
    np.testing.assert_array_equal(res.censored()[0, 0], [0, 1, 0, 0])
    assert res.mean_duration()[0, 0] == 8 / 3 and res.longest_spell_map()[0, 0, 0, 0] == 5
    assert res.mean_spell_map()[0, 0, 0, 0] == 8 / 3 and res.spell_frequency()[0, 0, 0, 0] == 3 / 13
    # durations 1, 2, >= 4: quantiles and survival by hand
    np.testing.assert_array_equal(res.duration_quantile([0.2, 1 / 3, 0.5, 2 / 3, 0.9, 1.0])[0, 0], [1, 1, 2, 2, 4, 4])
    assert res.duration_quantile(0.5)[0, 0] == 2
    np.testing.assert_array_equal(res.duration_survival()[0, 0], [1.0, 2 / 3, 1 / 3, 1 / 3])
    # the largest lag (20) >= T: it contributes nothing and is not an error
    assert st["ramps"][0, 1].sum() == 0 and st["accnt"][0, 2, 0] == 0 and st["ramps"][0, 0].sum() == 12
    assert st["ramps"][0, 0, -1] == 2                                # the two differences with the NaN
    r = res.autocorrelation()
    assert np.isfinite(r[0, 0, 0, 0]) and np.isnan(r[0, 1, 0, 0])
    # the "below" sense on the same data: y < 1 holds at time 10 only (NaN and equality fail)
    low = host_chunks(hand_spec(below=True), HAND.reshape(-1, 1, 1), cuts)
    np.testing.assert_array_equal(low["spells"][0, 0], [1, 0, 0, 0])
    np.testing.assert_array_equal(low["spellmap"][0, 0, :, 0], [1, 1, 1])
    assert low["open"][0, 0, 0] == 0


def test_constant_series_has_no_autocorrelation_and_an_empty_result_is_nan():
    spec = hand_spec(lags=(1, 2))
    st = temporal.host_temporal(spec, np.full((12, 1, 3), 2.5, dtype=F32))
    res = TemporalResult.from_state(spec, 1, 3, 12, st)
    assert np.isnan(res.autocorrelation()).all() and np.isnan(res.decorrelation_time()).all()
    np.testing.assert_array_equal(res.censored()[0, 0], [0, 0, 0, 3])     # three pixels with an open run of 12 >= ndur
    assert res.spell_counts().sum() == 0 and np.isnan(res.mean_duration()).all() and np.isnan(res.duration_quantile(0.5)).all()
    assert np.isnan(res.duration_survival()).all() and np.isnan(res.mean_spell_map()).all()
    np.testing.assert_array_equal(st["ramps"][0, :, 1 + 4], [11 * 3, 10 * 3])  # d = 0 falls in the bin that starts at 0
    json.dumps(res.summary(), allow_nan=False)


# ------------------------------------------------------------------------------------------------- TemporalResult on the host
def test_autocorrelation_against_numpy_float64():
    """|y| <= 8, T = 300, per-pixel variance >= 0.1: the summation-order error of the device's sums is about T * 64 * 2^-53 / 0.1
    ~ 2e-11; 1e-9 absolute covers the divisions."""
    rng = np.random.default_rng(11)
    T, H, W = 300, 3, 4
    spec = TemporalSpec(2, speed=(0, 1), thresholds=(), lags=(1, 2, 3, 6))
    x = np.empty((T, 2, H * W), dtype=F32)
    x[0] = rng.standard_normal((2, H * W))
    for t in range(1, T):
        x[t] = 0.7 * x[t - 1] + 0.7 * rng.standard_normal((2, H * W)).astype(F32)
    x = np.clip(x * 1.2, -5.0, 5.0)
    x[5, 0, 3] = np.nan                                              # one missing value: the pairs that hold it drop out
    y = y_ref(spec, x).astype(np.float64)                            # [T, nout, P]
    assert np.nanmax(np.abs(y)) <= 8 and np.nanvar(y, axis=0).min() >= 0.1
    res = TemporalResult.from_state(spec, H, W, T, temporal.host_temporal(spec, x))
    got = res.autocorrelation()
    want = np.empty((spec.nout, spec.nlag, H * W))
    for j in range(spec.nout):
        for p in range(H * W):
            v = y[:, j, p]
            ok = np.isfinite(v)
            mu, var = v[ok].mean(), v[ok].var()
            for l, tau in enumerate(spec.lags):
                a, b = v[tau:], v[:-tau]
                m = np.isfinite(a) & np.isfinite(b)
                want[j, l, p] = ((a[m] - mu) * (b[m] - mu)).mean() / var
    assert np.abs(got.reshape(want.shape) - want).max() <= 1e-9
    assert got.shape == (spec.nout, spec.nlag, H, W)
    two = TemporalResult.from_state(spec, H, W, T, temporal.host_temporal(spec, x), temporal.host_temporal(spec, x[::-1].copy()))
    np.testing.assert_array_equal(two.autocorrelation_bias(), two.autocorrelation("fake") - two.autocorrelation("real"))
    with pytest.raises(ValueError, match="paired"):
        res.autocorrelation_bias()
    with pytest.raises(ValueError, match="side"):
        res.autocorrelation("fake")


def test_decorrelation_time_by_hand():
    """Pixels whose autocorrelation at lags (1, 2, 4) is planted through the sums: n = m = 1, s1 = 0, s2 = 1 give r = c."""
    spec = TemporalSpec(1, speed=None, thresholds=(), lags=(1, 2, 4))
    r = np.array([[0.8, 0.5, 0.2], [0.3, 0.1, 0.0], [0.9, 0.8, 0.7], [0.9, np.nan, 0.1], [0.5, 0.5, 0.25]])   # [P, nlag]
    P = len(r)
    st = zero_state(spec, P)
    st["accnt"][0, 0] = 1
    st["acsum"][0, 1] = 1.0
    for l in range(3):
        st["accnt"][0, 1 + l] = np.where(np.isnan(r[:, l]), 0, 1)
        st["acsum"][0, 2 + 2 * l] = np.nan_to_num(r[:, l])
    res = TemporalResult.from_state(spec, 1, P, 1, st)
    np.testing.assert_allclose(res.autocorrelation()[0, :, 0].T, r, rtol=0, atol=0)
    got = res.decorrelation_time(level=0.4)[0, 0]
    # 0.5 -> 0.2 between lags 2 and 4; 1 -> 0.3 between lags 0 and 1; never; NaN before it is reached; exactly flat then down
    want = [2 + (0.5 - 0.4) / (0.5 - 0.2) * 2, (1 - 0.4) / (1 - 0.3), np.nan, np.nan, 2 + (0.5 - 0.4) / (0.5 - 0.25) * 2]
    np.testing.assert_allclose(got, want, rtol=1e-15, equal_nan=True)
    assert res.decorrelation_time().shape == (1, 1, P)


def test_ramp_histogram_is_a_histogram_and_results_save(tmp_path):
    name, spec = specs()[0]
    T, H, W = 40, 3, 3
    rng = np.random.default_rng(9)
    xa, xb = data(rng, spec, T, H * W), data(rng, spec, T, H * W)
    res = TemporalResult.from_state(spec, H, W, T, temporal.host_temporal(spec, xa), temporal.host_temporal(spec, xb))
    ha, hb = res.ramp_histogram("speed", 2), res.ramp_histogram(2, 2, "fake")
    np.testing.assert_array_equal(ha.host()[0][0], res.ramp_hist()[2, 1])
    assert -4.0 <= ha.quantile(0.5)[0] <= 4.0
    assert res.ramp_w1()[2, 1] == histograms.wasserstein1(ha, hb)[0] and res.ramp_ks()[2, 1] == histograms.ks_distance(ha, hb)[0]
    assert res.ramp_w1().shape == (3, 4) and (res.ramp_ks() <= 1).all()
    with pytest.raises(KeyError, match="lag"):
        res.ramp_histogram(0, 5)
    names = res.save(str(tmp_path / "t"))
    want = {f"{s}_{k}.npy" for s in ("real", "fake") for k in ("spell_frequency", "mean_spell", "longest_spell", "autocorrelation",
                                                               "decorrelation_time", "spells", "censored", "ramps")}
    assert set(names) == want | {"autocorrelation_bias.npy", "summary.json"} and all(os.path.exists(tmp_path / "t" / n) for n in names)
    assert np.load(tmp_path / "t" / "autocorrelation_bias.npy").shape == (3, 4, H, W)
    assert set(res.maps()) == {n[:-4] for n in names if n.endswith(".npy") and n.split("_", 1)[1][:-4] not in ("spells", "censored", "ramps")}
    s = json.load(open(tmp_path / "t" / "summary.json"))
    assert s == json.loads(json.dumps(res.summary(), allow_nan=False))
    assert s["channels"] == ["ch0", "ch1", "speed"] and s["fields"] == T and s["lags"] == [1, 2, 3, 24] and s["series"] == ["real", "fake"]
    assert np.array(s["real"]["spells"]).shape == (3, 4) and np.array(s["ramp_w1"]).shape == (3, 4)


# ------------------------------------------------------------------------------------------------- checks before any library call
def test_spec_defaults_and_struct():
    z = TemporalSpec.zscore(2)
    assert z.nout == 3 and z.names == ["ch0", "ch1", "speed"] and z.lags == (1, 2, 3, 6) and z.R == 6 and z.nthr == 4
    assert z.below == (False, False, True, True) and z.thresholds[0].tolist() == [1.0, 2.0, -1.0, -2.0]
    assert z.thresholds[2].tolist() == [1.5, 2.5, 0.5, 0.25] and (z.lo == -z.ranges).all() and z.ranges[0, 0] == 8.0
    one = TemporalSpec.zscore(1)
    assert one.nout == 1 and one.speed is None
    s = z.struct()
    assert (s.speed_u, s.speed_v, s.nthr, s.ndur, s.nlag, s.nbins) == (0, 1, 4, 64, 4, 128)
    assert list(s.below) == [0, 0, 1, 1] and list(s.lag) == [1, 2, 3, 6] and s.thr[2][1] == 2.5 and s.inv_w[2][3] == 8.0
    assert z == TemporalSpec.zscore(2) and z != TemporalSpec.zscore(2, ndur=8)
    assert z.shapes(2, 10)["tail"] == ((2, 3, 6, 10), np.float32) and z.shapes(1, 10)["acsum"] == ((1, 3, 10, 10), np.float64)
    assert (temporal.THR_MAX, temporal.DUR_MAX, temporal.LAGS_MAX, temporal.LAG_MAX, temporal.BINS_MAX) == (4, 256, 4, 24, 512)
    assert "reduce_" not in dir(Temporal) and "interleaved" in Temporal.__doc__


@pytest.mark.parametrize("kw,match", [
    (dict(C=0), "C <="), (dict(C=9), "C <="), (dict(C=1), "speed"), (dict(speed=(0, 2)), "speed"),
    (dict(scale=[1.0]), "scale"), (dict(offset=[float("nan"), 0.0]), "finite"),
    (dict(thresholds=[1.0] * 5), "at most 4"), (dict(thresholds=[[1.0], [1.0]]), "one list per output channel"),
    (dict(thresholds=[float("inf")]), "finite"), (dict(thresholds=[1.0, 2.0], below=[True]), "one flag per threshold"),
    (dict(ndur=0), "ndur"), (dict(ndur=257), "ndur"), (dict(lags=(1, 2, 3, 4, 5)), "at most 4"), (dict(lags=(0,)), "lags"),
    (dict(lags=(25,)), "lags"), (dict(lags=(2, 2)), "increasing"), (dict(lags=(3, 1)), "increasing"),
    (dict(lags=(), thresholds=()), "at least one"), (dict(nbins=0), "nbins"), (dict(nbins=513), "nbins"),
    (dict(ranges=0.0), "> 0"), (dict(ranges=[1.0, 2.0]), "ranges"), (dict(ranges=1e-40), "fp32 range"),
    (dict(names=["a"]), "names"),
])
def test_spec_rejects(kw, match):
    with pytest.raises(ValueError, match=match):
        TemporalSpec(**dict(dict(C=2, thresholds=[1.0]), **kw))


def test_arguments_are_checked_before_any_library_call(monkeypatch):
    _no_library(monkeypatch)
    spec = TemporalSpec.zscore(2)
    with pytest.raises(TypeError, match="TemporalSpec"):
        Temporal(object(), 8, 8, device="cpu")
    with pytest.raises(ValueError, match="grid"):
        Temporal(spec, 0, 8, device="cpu")
    pair, single = Temporal(spec, 8, 8, device="cpu"), Temporal(spec, 8, 8, paired=False, device="cpu")
    x = torch.zeros(3, 2, 8, 8)
    for call, match in ((lambda: pair.add(x), "paired"), (lambda: single.add(x, x), "one series"),
                        (lambda: single.add(torch.zeros(3, 3, 8, 8)), "C = 2"), (lambda: single.add(torch.zeros(3, 2, 8, 4)), "grid"),
                        (lambda: pair.add(x, torch.zeros(2, 2, 8, 8)), "differ in length"), (lambda: single.add(x, n_valid=4), "n_valid"),
                        (lambda: single.add(x, n_valid=0), "n_valid"), (lambda: single.add(x, nhwc=(True, False, True)), "nhwc"),
                        (lambda: temporal.temporal(x, spec=TemporalSpec.zscore(3)), "C = 3"),
                        (lambda: temporal.host_temporal(spec, np.zeros((3, 3, 4), F32)), "C = 2"),
                        (lambda: temporal.host_temporal(spec, np.zeros((3, 2, 4), F32), t0=-1), "2\\^31"),
                        (lambda: temporal.host_temporal(spec, np.zeros((3, 2, 4), F32), t0=2 ** 31 - 3), "2\\^31"),
                        (lambda: temporal.host_temporal(spec, np.zeros((3, 2, 4), F32), state=zero_state(spec, 5)), "state")):
        with pytest.raises(ValueError, match=match):
            call()
    for call in (lambda: single.add(x.double()), lambda: temporal.temporal(x, spec=object()), lambda: temporal.host_temporal(None, x)):
        with pytest.raises(TypeError):
            call()
    full = Temporal(spec, 2, 2, paired=False, device="cpu")
    full.fields = 2 ** 31 - 3
    with pytest.raises(ValueError, match="2\\^31"):
        full.add(torch.zeros(3, 2, 2, 2))
    assert single.fields == 0 and pair.fields == 0
    # nbytes: S * nout * P * (4 nthr + 4 R + 12 nthr + 8 (2 + 2 nlag) + 4 (1 + nlag)) + the two pooled tables
    P = 64
    assert pair.nbytes == 2 * 3 * P * (16 + 24 + 48 + 80 + 20) + 2 * 3 * (4 * 64 + 4 * 131) * 8


# ------------------------------------------------------------------------------------------------- the ABI
def test_header_declares_and_library_exports_the_temporal_abi(tmp_path):
    src = open(os.path.join(ROOT, "include", "downgan_hip.h")).read()
    assert "Temporal diagnostics (csrc/temporal.hip)" in src and "LEFT-CENSORED" in src
    for name, v in (("THR", 4), ("DUR", 256), ("LAGS", 4), ("LAG", 24), ("BINS", 512)):
        assert re.search(rf"#define DG_TEMPORAL_MAX_{name} {v}\b", src), name
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    ctype = {"const dg_eof_fields*": C.POINTER(_lib.EofFields), "const dg_temporal_spec*": C.POINTER(_lib.TemporalSpec), "int": C.c_int,
             "int64_t": C.c_int64}
    for sym in ("dg_temporal_ws_bytes", "dg_temporal", "dg_temporal_host"):
        m = re.search(rf"\b(size_t|int) {sym}\s*\(([^)]*)\)", code)
        assert m, sym
        assert sym in _lib.EXPORTS and hasattr(_lib.lib(), sym)
        args = [" ".join(a.split()[:-1]) for a in m.group(2).replace("\n", " ").split(",")]
        want = [ctype.get(a, C.c_void_p) for a in args]                 # every other pointer is passed as void*
        assert _lib._PROTOS[sym] == want, (sym, args)
        assert getattr(_lib.lib(), sym).restype == (C.c_size_t if m.group(1) == "size_t" else C.c_int)
    assert "temporal.hip" in open(os.path.join(ROOT, "downgan_amd", "csrc", "Makefile")).read()
    # sizeof / offsetof of dg_temporal_spec, compiled as plain C
    cls = _lib.TemporalSpec
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{ROOT}/include/downgan_hip.h"', 'int main(void) {',
             '  printf("size %zu\\n", sizeof(dg_temporal_spec));']
    lines += [f'  printf("{f} %zu\\n", offsetof(dg_temporal_spec, {f}));' for f, _ in cls._fields_]
    (tmp_path / "layout.c").write_text("\n".join(lines + ['  return 0;', '}']))
    subprocess.run(["gcc", "-std=c99", "-o", str(tmp_path / "layout"), str(tmp_path / "layout.c")], check=True)
    got = dict(l.split() for l in subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["size"]) == C.sizeof(cls)
    for f, _ in cls._fields_:
        assert int(got[f]) == getattr(cls, f).offset, f


def test_abi_rejects_bad_arguments_without_launching():
    lib = _lib.lib()
    ok = dict(base=0x1000, dtype=_lib.DG_F32, T=64, C=2, P=100, ld_t=200, ld_c=100, ld_p=1)
    f = lambda **kw: C.byref(_lib.EofFields(**dict(ok, **kw)))
    base = TemporalSpec.zscore(2)
    good = C.byref(base.struct())

    def spec(**kw):
        s = base.struct()
        for k, v in kw.items():
            if isinstance(v, tuple) and len(v) == 3:
                getattr(s, k)[v[0]][v[1]] = v[2]
            elif isinstance(v, tuple):
                getattr(s, k)[v[0]] = v[1]
            else:
                setattr(s, k, v)
        return C.byref(s)
    p = C.c_void_p(0x3000)
    names = ("a", "b", "s", "t0", "ws", "open", "tail", "spells", "spellmap", "ramps", "acsum", "accnt", "stream")
    dflt = dict(a=f(), b=None, s=good, t0=0, ws=None, open=p, tail=p, spells=p, spellmap=p, ramps=p, acsum=p, accnt=p, stream=None)
    call = lambda **kw: lib.dg_temporal(*[dict(dflt, **kw)[k] for k in names])
    nan, inf = float("nan"), float("inf")
    bad = [dict(a=None), dict(a=f(base=0)), dict(s=None), dict(open=None), dict(tail=None), dict(spells=None), dict(spellmap=None),
           dict(ramps=None), dict(acsum=None), dict(accnt=None), dict(a=f(C=9)), dict(a=f(T=0)), dict(a=f(P=0)),
           dict(b=f(T=63)), dict(b=f(P=96)), dict(b=f(base=0)), dict(a=f(C=3), b=f(C=2)),
           dict(s=spec(nthr=-1)), dict(s=spec(nthr=5)), dict(s=spec(ndur=0)), dict(s=spec(ndur=257)), dict(s=spec(nlag=-1)),
           dict(s=spec(nlag=5)), dict(s=spec(nbins=0)), dict(s=spec(nbins=513)), dict(s=spec(nthr=0, nlag=0)),
           dict(s=spec(below=(1, 2))), dict(s=spec(lag=(0, 0))), dict(s=spec(lag=(3, 25))), dict(s=spec(lag=(1, 1))),
           dict(s=spec(lag=(2, 1))), dict(s=spec(thr=(2, 1, nan))), dict(s=spec(thr=(0, 0, inf))), dict(s=spec(lo=(2, 3, nan))),
           dict(s=spec(inv_w=(0, 0, inf))), dict(s=spec(inv_w=(1, 2, 0.0))), dict(s=spec(inv_w=(1, 2, -1.0))),
           dict(s=spec(scale=(1, inf))), dict(s=spec(offset=(0, nan))), dict(s=spec(speed_u=2)), dict(s=spec(speed_v=-1)),
           dict(a=f(C=1)),                                           # speed channel 1 of a 1-channel field
           dict(t0=-1), dict(t0=2 ** 31 - 64), dict(t0=2 ** 31), dict(t0=2 ** 40)]
    for kw in bad:
        assert call(**kw) == -1, kw
    assert call(a=f(dtype=7)) == -2 and call(b=f(dtype=7)) == -2
    assert lib.dg_temporal_ws_bytes(f(), None, spec(nbins=513)) == 0 and lib.dg_temporal_ws_bytes(f(), f(T=63), good) == 0
    assert lib.dg_temporal_ws_bytes(None, None, good) == 0 and 0 < lib.dg_temporal_ws_bytes(f(), f(), good) <= 4096
    hnames = ("s", "x", "C", "T", "P", "t0", "open", "tail", "spells", "spellmap", "ramps", "acsum", "accnt")
    hd = dict(s=good, x=p, C=2, T=4, P=4, t0=0, open=p, tail=p, spells=p, spellmap=p, ramps=p, acsum=p, accnt=p)
    host = lambda **kw: lib.dg_temporal_host(*[dict(hd, **kw)[k] for k in hnames])
    for kw in (dict(s=None), dict(x=None), dict(C=0), dict(C=9), dict(T=0), dict(P=0), dict(t0=-1), dict(t0=2 ** 31 - 4), dict(open=None),
               dict(tail=None), dict(spells=None), dict(spellmap=None), dict(ramps=None), dict(acsum=None), dict(accnt=None),
               dict(s=spec(lag=(3, 25))), dict(s=spec(below=(0, -1))), dict(C=1)):
        assert host(**kw) == -1, kw


# ------------------------------------------------------------------------------------------------- trainer hook, emulated
def temporal_emu_ops(calls=None):
    from oracle.emu_ops import EmuOps

    class TemporalEmuOps(EmuOps):
        """The emulated ops plus dg_temporal's contract in numpy (``temporal_ref`` per series on the state tensors)."""

        def __getattribute__(self, name):
            v = object.__getattribute__(self, name)
            if calls is not None and callable(v) and not name.startswith("_"):
                calls.append(name)
            return v

        @staticmethod
        def eof_fields(t, nhwc=False, channels=None):
            Cn = (t.shape[3] if channels is None else channels) if nhwc else t.shape[1]
            P = t.shape[1] * t.shape[2] if nhwc else t.shape[2] * t.shape[3]
            return types.SimpleNamespace(t=t, nhwc=nhwc, T=t.shape[0], C=Cn, P=P)

        def temporal_ws_bytes(self, fa, fb, spec):
            return 1

        def temporal(self, fa, fb, s, t0, open_, tail, spells, spellmap, ramps, acsum, accnt):
            def values(f):
                x = f.t[..., :f.C].permute(0, 3, 1, 2) if f.nhwc else f.t[:, :f.C]
                return np.ascontiguousarray(x.detach().float().cpu().numpy().reshape(f.T, f.C, -1))
            nout = fa.C + (s.speed_u >= 0)
            spec = TemporalSpec(fa.C, scale=list(s.scale[:fa.C]), offset=list(s.offset[:fa.C]),
                                speed=None if s.speed_u < 0 else (s.speed_u, s.speed_v),
                                thresholds=[list(s.thr[j][:s.nthr]) for j in range(nout)], below=[bool(b) for b in s.below[:s.nthr]],
                                ndur=s.ndur, lags=list(s.lag[:s.nlag]), nbins=s.nbins,
                                ranges=[[-s.lo[j][l] for l in range(s.nlag)] for j in range(nout)])
            assert np.array_equal(spec.inv_w, np.array([list(s.inv_w[j][:s.nlag]) for j in range(nout)], F32).reshape(nout, s.nlag))
            arrays = dict(zip(ARRAYS, (open_, tail, spells, spellmap, ramps, acsum, accnt)))
            for ser, f in enumerate((fa,) if fb is None else (fa, fb)):
                temporal_ref(spec, values(f), int(t0), {k: v[ser].numpy() for k, v in arrays.items()})   # views: updated in place

    return TemporalEmuOps("f32")


def _trainer(on, dist=None, fs=False, tdir=None):
    from downgan_amd.GAN.wasserstein import WassersteinGAN
    from downgan_amd.GAN.wasserstein_fs import WassersteinGANFS
    from downgan_amd.networks.critic import Critic
    from downgan_amd.networks.generator import Generator
    G, C_ = Generator(16, 128, 2, 2, num_res_blocks=1), Critic(16, 128, 2)
    tr = (WassersteinGANFS if fs else WassersteinGAN)(G, C_, dist=dist)
    tr.log_temporal = on
    tr.temporal_dir = tdir
    tr.temporal_spec = TemporalSpec(2, speed=(0, 1), thresholds=[0.5, -0.5], below=(False, True), ndur=4, lags=(1, 3), nbins=16,
                                    ranges=4.0)
    return tr


def _patch(setattr_, calls=None):
    from downgan_amd import backend
    from downgan_amd.GAN import losses
    setattr_(backend, "make_ops", lambda dtype, device: temporal_emu_ops(calls))
    setattr_(losses, "_ops", {})
    setattr_(histograms, "_ops", {})


def _loaders(batch=2):
    from downgan_amd import synthetic
    from downgan_amd.GAN.dataloader import NetCDFSR
    coarse, fine = synthetic.tiles(6, 2, 16, seed=11)
    ds = lambda a, b: NetCDFSR(torch.from_numpy(coarse[a:b].copy()), torch.from_numpy(fine[a:b].copy()))
    return torch.utils.data.DataLoader(ds(0, 2), batch_size=batch), torch.utils.data.DataLoader(ds(2, 6), batch_size=batch)


def _run_epoch(on, dist=None, fs=False, tdir=None):
    torch.manual_seed(0)                                  # initial weights, the gradient penalty's alpha
    tr = _trainer(on, dist, fs, tdir)
    dl, tl = _loaders()
    tr.train(dl, tl, epochs=1)
    return tr


def test_hook_off_leaves_the_summary_and_the_calls_unchanged(monkeypatch, tmp_path):
    import downgan_amd.config.hyperparams as hp
    from downgan_amd.engine import TrainEngine
    from downgan_amd.GAN.wasserstein import WassersteinGAN
    calls = []
    _patch(monkeypatch.setattr, calls)
    monkeypatch.setattr(hp, "batch_size", 2)
    torch.set_num_threads(4)
    assert WassersteinGAN.log_temporal is False and WassersteinGAN.temporal_spec is None
    assert WassersteinGAN.temporal_dir is None and WassersteinGAN.temporal_results is None
    seen = []
    real_pass = TrainEngine.metrics_pass

    def spy(self, *a, **kw):
        seen.append(set(kw))
        return real_pass(self, *a, **kw)
    monkeypatch.setattr(TrainEngine, "metrics_pass", spy)
    t_off = _run_epoch(False)
    off, calls_off = t_off.metrics_log[0], list(calls)
    assert "temporal" not in off and t_off.temporal_results is None
    assert len(seen) == 3 and not any("temporal" in kw for kw in seen)      # the new keyword is handed down only when the hook is on
    assert "temporal" not in calls_off and "eof_fields" not in calls_off
    del seen[:], calls[:]
    tr = _run_epoch(True, tdir=str(tmp_path / "t"))
    assert ["temporal" in kw for kw in seen] == [False, True, True]        # the train batch, then the two test batches
    assert [c for c in calls if c not in ("temporal", "eof_fields", "temporal_ws_bytes")] == calls_off
    assert calls.count("temporal") == 2
    on = dict(tr.metrics_log[0])
    d = on.pop("temporal")
    assert json.dumps(on, sort_keys=True) == json.dumps(off, sort_keys=True)    # the hook adds a key and changes nothing else
    json.dumps(d, allow_nan=False)
    assert set(d) == {"test"} == set(tr.temporal_results)
    res = tr.temporal_results["test"]
    assert d["test"] == res.summary() and d["test"]["fields"] == 4 == res.fields and d["test"]["grid"] == [128, 128]
    assert d["test"]["channels"] == ["ch0", "ch1", "speed"] and d["test"]["lags"] == [1, 3] and d["test"]["series"] == ["real", "fake"]
    assert os.path.exists(tmp_path / "t" / "0" / "test" / "summary.json")
    assert np.load(tmp_path / "t" / "0" / "test" / "autocorrelation_bias.npy").shape == (3, 2, 128, 128)
    # the real side of the pair is the test set, in the loader's order, as one series of four times
    from downgan_amd import synthetic
    _, fine = synthetic.tiles(6, 2, 16, seed=11)
    want = TemporalResult.from_state(tr.temporal_spec, 128, 128, 4, temporal.host_temporal(tr.temporal_spec, fine[2:6].reshape(4, 2, -1)))
    for k in ("spells", "cens", "spellmap", "ramps", "accnt"):
        np.testing.assert_array_equal(getattr(res, k)[0], getattr(want, k)[0], err_msg=k)
    np.testing.assert_array_equal(res.acsum[0].view(np.uint64), want.acsum[0].view(np.uint64))
    assert res.ramps[1].sum() == res.ramps[0].sum() == 3 * 128 * 128 * (3 + 1)


def test_hook_without_log_metrics(monkeypatch):
    import downgan_amd.config.hyperparams as hp
    _patch(monkeypatch.setattr)
    monkeypatch.setattr(hp, "batch_size", 2)
    torch.set_num_threads(4)
    from downgan_amd.GAN.wasserstein import WassersteinGAN
    monkeypatch.setattr(WassersteinGAN, "log_metrics", False)
    s = _run_epoch(True).metrics_log[0]
    assert "train" not in s and "test" not in s and set(s["temporal"]) == {"test"} and s["temporal"]["test"]["fields"] == 4


def test_frequency_separation_trainer_reports_temporal(monkeypatch):
    import downgan_amd.config.hyperparams as hp
    _patch(monkeypatch.setattr)
    monkeypatch.setattr(hp, "batch_size", 2)
    torch.set_num_threads(4)
    s = _run_epoch(True, fs=True).metrics_log[0]
    assert set(s["temporal"]) == {"test"} and s["temporal"]["test"]["fields"] == 4


def test_data_parallel_world_raises_before_anything_is_accumulated(monkeypatch):
    calls = []
    _patch(monkeypatch.setattr, calls)
    tr = _trainer(True, dist=types.SimpleNamespace(world_size=2, rank=0))
    dl, tl = _loaders()
    with pytest.raises(ValueError, match="one rank"):
        tr._train_epoch(dl, tl)
    assert calls == [] and tr.temporal_results is None and tr.metrics_log == [] and tr.num_steps == 0
