"""The trainer's plumbing of the twelve opt-in per-epoch diagnostics, without a GPU and without a diagnostic kernel: every
accumulator class is replaced in its own module by a recording stub (the trainer imports them lazily), the ops are the
emulated ones.  What is pinned: which constructor gets which spec, grid and device; the ``add`` calls of every metrics pass,
their order and arguments; the summary keys and their order; the ``*_results`` attributes; who saves where; the test-loader
walk without ``log_metrics``; and that nothing is constructed while every flag is off."""
import json
import os
import subprocess
import sys
import types

import pytest
import torch

from downgan_amd import (distmap, fss, gridhist, gridstats, histograms, increments, joint, objects, spectra, temporal)

FLAGS = ("log_spectra", "log_distributions", "log_maps", "log_fss", "log_joint", "log_coherence", "log_increments",
         "log_quantile_maps", "log_temporal", "log_helmholtz", "log_objects", "log_distances")
KEYS = ("spectra", "distributions", "maps", "fss", "joint", "coherence", "increments", "quantile_maps", "temporal", "helmholtz",
        "objects", "distances")                                          # the summary keys, in the summary's order
RESULTS = {"distributions": "distribution_results", "maps": "map_results", "fss": "fss_results", "joint": "joint_results",
           "increments": "increment_results", "quantile_maps": "quantile_map_results", "temporal": "temporal_results",
           "objects": "objects_results", "distances": "distance_results"}
# the order in which one metrics pass feeds its sinks (metrics_pass keyword, which of the pass's tensors each add receives)
FEED = (("spectra", 0, ("fine",)), ("spectra", 1, ("fake",)), ("coherence", None, ("fine", "fake")),
        ("helmholtz", None, ("fine", "fake")), ("distributions", 0, ("fine",)), ("distributions", 1, ("fake",)),
        ("maps", None, ("fine", "fake")), ("fss", None, ("fine", "fake")), ("joint", None, ("fine", "fake")),
        ("increments", None, ("fine", "fake")), ("hist_maps", None, ("fine", "fake")), ("temporal", None, ("fine", "fake")),
        ("objects", None, ("fine", "fake")), ("distances", None, ("fine", "fake")))
K = 65                                                                   # rings of a 128 x 128 field


class Log:
    def __init__(self):
        self.made = []       # (class name, stub, args, kwargs) of every constructor call
        self.passes = []     # one dict per TrainEngine.metrics_pass: engine, fine, kw, adds = [(stub, tensors, kwargs)]
        self.reduced = []    # (stub, dist)
        self.saved = []      # (result, args)
        self.summarised = []  # (result, args)

    def of(self, name):
        return [m for m in self.made if m[0] == name]


class Result:
    """A canned result: summary() and save() record their arguments."""

    def __init__(self, log, acc):
        self.log, self.acc = log, acc

    def summary(self, *args):
        self.log.summarised.append((self, args))
        return {"stub": self.acc.name, "serial": self.acc.serial, "args": [list(a) for a in args]}

    def save(self, *args):
        self.log.saved.append((self, args))


def _stub(log, name):
    class Stub:
        def __init__(self, *args, **kw):
            self.name, self.serial, self.args, self.kw = name, len(log.made), args, kw
            self.count, self.N = 7, 128
            self.res = Result(log, self)
            log.made.append((name, self, args, kw))

        def add(self, *tensors, **kw):
            log.passes[-1]["adds"].append((self, tensors, kw))
            return self

        def reduce_(self, dist):
            log.reduced.append((self, dist))
            return self

        def result(self):
            if name == "ValueHistogram":                                 # a real Histogram over canned host counts
                spec = self.args[0]
                counts = torch.zeros(spec.nout, spec.bins + 3, dtype=torch.int64)
                counts[:, 1:-2] = 1 + self.serial % 2
                n = float(counts[0].sum())
                return histograms.Histogram(spec, counts, torch.tensor([[0.0, n]] * spec.nout, dtype=torch.float64),
                                            torch.tensor([[-1.0, 1.0]] * spec.nout), 5)
            return self.res

        def mean(self):
            shape = {"RadialSpectrum": (2, K), "CrossSpectrum": (2, 3, K), "HelmholtzSpectrum": (8, K)}[name]
            t = torch.full(shape, 2.0, dtype=torch.float64)
            if name == "CrossSpectrum":
                t[:, 2] = 1.0                                            # coherence 0.5 on every ring
            return t
    Stub.__name__ = name
    return Stub


STUBBED = ((spectra, "RadialSpectrum"), (spectra, "CrossSpectrum"), (spectra, "HelmholtzSpectrum"), (histograms, "ValueHistogram"),
           (gridstats, "GridStats"), (fss, "FractionsSkill"), (joint, "ValueJoint"), (increments, "Increments"),
           (gridhist, "GridHist"), (temporal, "Temporal"), (objects, "Objects"), (distmap, "Distances"))


@pytest.fixture
def log(monkeypatch):
    import downgan_amd.config.hyperparams as hp
    from downgan_amd import backend
    from downgan_amd.engine import TrainEngine
    from downgan_amd.GAN import losses
    from oracle.emu_ops import EmuOps
    monkeypatch.setattr(backend, "make_ops", lambda dtype, device: EmuOps("f32"))
    monkeypatch.setattr(losses, "_ops", {})
    monkeypatch.setattr(histograms, "_ops", {})
    monkeypatch.setattr(hp, "batch_size", 2)
    torch.set_num_threads(4)
    lg = Log()
    for mod, name in STUBBED:
        monkeypatch.setattr(mod, name, _stub(lg, name))
    real_pass = TrainEngine.metrics_pass

    def spy(self, coarse, fine, **kw):
        lg.passes.append({"engine": self, "fine": fine, "kw": kw, "adds": []})
        return real_pass(self, coarse, fine, **kw)
    monkeypatch.setattr(TrainEngine, "metrics_pass", spy)
    return lg


def _trainer(on=None, dist=None, **attrs):
    from downgan_amd.GAN.wasserstein import WassersteinGAN
    from downgan_amd.networks.critic import Critic
    from downgan_amd.networks.generator import Generator
    tr = WassersteinGAN(Generator(16, 128, 2, 2, num_res_blocks=1), Critic(16, 128, 2), dist=dist)
    if on is not None:
        for flag in FLAGS:
            setattr(tr, flag, on)
    for k, v in attrs.items():
        setattr(tr, k, v)
    return tr


class CountingLoader:
    """A DataLoader that counts how often it is walked."""

    def __init__(self, dl):
        self.dl, self.walks = dl, 0

    def __iter__(self):
        self.walks += 1
        return iter(self.dl)


def _loaders():
    from downgan_amd import synthetic
    from downgan_amd.GAN.dataloader import NetCDFSR
    coarse, fine = synthetic.tiles(6, 2, 16, seed=11)
    ds = lambda a, b: NetCDFSR(torch.from_numpy(coarse[a:b].copy()), torch.from_numpy(fine[a:b].copy()))
    return torch.utils.data.DataLoader(ds(0, 2), batch_size=2), CountingLoader(torch.utils.data.DataLoader(ds(2, 6), batch_size=2))


def _run(tr, epochs=1):
    torch.manual_seed(0)                                  # initial weights, the gradient penalty's alpha
    dl, tl = _loaders()
    tr.train(dl, tl, epochs=epochs)
    return tl


def _check_passes(log, parts=("train", "test", "test")):
    """Every pass fed the enabled sinks of its part in FEED's order, with the pass's own tensors and the common keywords."""
    assert len(log.passes) == len(parts)
    for p, part in zip(log.passes, parts):
        fake = p["engine"].G.fake
        named = {id(p["fine"]): "fine", id(fake): "fake"}
        want = [(p["kw"][k] if i is None else p["kw"][k][i], which) for k, i, which in FEED if part == "test" or k != "temporal"]
        assert len(want) == (14 if part == "test" else 13) and ("temporal" in p["kw"]) == (part == "test")
        assert [(a[0], tuple(named.get(id(t)) for t in a[1])) for a in p["adds"]] == want
        assert all(a[2] == {"n_valid": 2, "nhwc": True, "channels": 2} for a in p["adds"])


def test_all_hooks_on_construct_feed_summarise_and_save(log, tmp_path):
    dirs = {k: str(tmp_path / k) for k in ("map_dir", "quantile_map_dir", "temporal_dir")}
    tr = _trainer(True, **dirs)
    tl = _run(tr)
    assert tl.walks == 1
    _check_passes(log)
    # ---- constructors: two parts each (temporal: the test part only), the default specs, the fine grid, the ops' device
    cpu = torch.device("cpu")
    grid = (128, 128)
    H = histograms.HistSpec
    want = {"RadialSpectrum": (4, (2, 128), {}), "CrossSpectrum": (2, (2, 128), {}),
            "HelmholtzSpectrum": (2, (128,), {"pair": (0, 1), "scale": None, "rows_up": True}),
            "ValueHistogram": (4, (H.zscore(2),), {}), "GridStats": (2, (gridstats.GridSpec.zscore(2),) + grid, {"paired": True}),
            "FractionsSkill": (2, (fss.FssSpec.zscore(2),) + grid, {}), "ValueJoint": (2, (joint.JointSpec.zscore(2),), {}),
            "Increments": (2, (increments.IncrementSpec.zscore(2),), {}),
            "GridHist": (2, (H.zscore(2, bins=64, lim=6.0),) + grid, {"paired": True}),
            "Temporal": (1, (temporal.TemporalSpec.zscore(2),) + grid, {"paired": True}),
            "Objects": (2, (objects.ObjectSpec.zscore(2),) + grid, {"paired": True}),
            "Distances": (2, (distmap.DistSpec.zscore(2),) + grid, {})}
    assert len(log.made) == sum(n for n, _, _ in want.values()) == 27
    for name, (n, args, kw) in want.items():
        made = log.of(name)
        assert len(made) == n, name
        for _, _, a, k in made:
            assert a == args and k == dict(kw, device=cpu), name
    # ---- the summary: its keys in order, one entry per part, the stubs' own results kept per part
    s = tr.metrics_log[0]
    assert list(s) == ["epoch", "train", "test", "test_batches"] + list(KEYS)
    train, test = log.passes[0]["kw"], log.passes[1]["kw"]
    assert log.passes[2]["kw"].keys() == test.keys() and all(log.passes[2]["kw"][k] is test[k] for k in test)
    for key in KEYS:
        assert list(s[key]) == (["test"] if key == "temporal" else ["train", "test"]), key
    for key, attr in RESULTS.items():
        kw = "hist_maps" if key == "quantile_maps" else key
        for part, accs in (("train", train), ("test", test)):
            if key == "temporal" and part == "train":
                continue
            got = getattr(tr, attr)[part]
            if key == "distributions":
                assert [type(h) for h in got] == [histograms.Histogram] * 2 and got[0].spec == H.zscore(2)
                assert s[key][part]["fields"] == 5 and s[key][part]["q"] == list(tr.distribution_q)
                assert s[key][part]["exceed_q"] == list(tr.distribution_exceed_q) and s[key][part]["w1"] == [0.0] * 3
            else:
                assert got is accs[kw].res, (key, part)
                args = [[0.5, 0.95, 0.99]] if key == "quantile_maps" else []
                assert s[key][part] == {"stub": accs[kw].name, "serial": accs[kw].serial, "args": args}
        assert set(getattr(tr, attr)) == set(s[key])
    for part, accs in (("train", train), ("test", test)):
        assert s["spectra"][part]["fields"] == 7 and s["spectra"][part]["lsd"] == [0.0, 0.0]
        assert torch.tensor(s["spectra"][part]["real"]).shape == (2, K)
        c = s["coherence"][part]
        assert c["k_eff"] == [64, 64] and c["wavelength_px"] == [2.0, 2.0] and c["fields"] == 7 and c["coherence"] == [[0.5] * K] * 2
        h = s["helmholtz"][part]
        assert h["k_eff_rot"] == h["k_eff_div"] == 64 and h["fields"] == 7 and h["ke_real"] == [2.0] * K and h["coh_rot"] == [1.0] * K
    # ---- every accumulator but the temporal one was reduced over the trainer's dist, once
    reduced = [a for a, d in log.reduced if d is None]
    assert len(reduced) == len(log.reduced) == 26 and len(set(map(id, reduced))) == 26
    assert not any(a.name == "Temporal" for a in reduced)
    # ---- saves: maps, quantile maps (with q) and temporal under <dir>/<epoch>/<part>
    saved = {(r.acc.name, a) for r, a in log.saved}
    assert len(log.saved) == 5 and saved == {
        ("GridStats", (os.path.join(dirs["map_dir"], "0", "train"),)), ("GridStats", (os.path.join(dirs["map_dir"], "0", "test"),)),
        ("GridHist", (os.path.join(dirs["quantile_map_dir"], "0", "train"), (0.5, 0.95, 0.99))),
        ("GridHist", (os.path.join(dirs["quantile_map_dir"], "0", "test"), (0.5, 0.95, 0.99))),
        ("Temporal", (os.path.join(dirs["temporal_dir"], "0", "test"),))}


def test_custom_specs_reach_their_constructors_and_only_rank_zero_saves_maps(log, tmp_path):
    dirs = {k: str(tmp_path / k) for k in ("map_dir", "quantile_map_dir", "temporal_dir")}
    fspec = fss.FssSpec(2, speed=None, thresholds=(0.5,), scales=(1, 7))
    qspec = histograms.HistSpec.zscore(2, bins=16, lim=3.0)
    dist = types.SimpleNamespace(world_size=1, rank=1)
    tr = _trainer(True, dist=dist, fss_spec=fspec, quantile_map_spec=qspec, quantile_map_q=(0.1, 0.9), **dirs)
    _run(tr)
    _check_passes(log)
    assert all(a[0] is fspec for _, _, a, _ in log.of("FractionsSkill")) and len(log.of("FractionsSkill")) == 2
    assert all(a[0] is qspec for _, _, a, _ in log.of("GridHist")) and len(log.of("GridHist")) == 2
    assert all(d is dist for _, d in log.reduced) and len(log.reduced) == 26
    assert [(r.acc.name, a) for r, a in log.saved] == [("Temporal", (os.path.join(dirs["temporal_dir"], "0", "test"),))]
    s = tr.metrics_log[0]
    assert s["quantile_maps"]["test"]["args"] == [[0.1, 0.9]] and s["maps"]["test"]["args"] == []
    assert set(tr.map_results) == set(tr.quantile_map_results) == {"train", "test"}


def test_without_log_metrics_the_test_loader_is_still_walked_once(log):
    tr = _trainer(True, log_metrics=False)
    tl = _run(tr)
    assert tl.walks == 1
    _check_passes(log)
    s = tr.metrics_log[0]
    assert list(s) == ["epoch"] + list(KEYS)
    assert all(list(s[k]) == (["test"] if k == "temporal" else ["train", "test"]) for k in KEYS)


def test_all_flags_off_constructs_nothing_and_leaves_the_summary_unchanged(log):
    from downgan_amd.GAN.wasserstein import WassersteinGAN
    assert not any(getattr(WassersteinGAN, f) for f in FLAGS)
    assert all(getattr(WassersteinGAN, a) is None for a in RESULTS.values())
    bare = _trainer(None)
    _run(bare)
    off = _trainer(False)
    _run(off)
    assert log.made == [] and len(log.passes) == 6
    assert all(p["adds"] == [] and all(v is None for v in p["kw"].values()) for p in log.passes)
    a, b = bare.metrics_log[0], off.metrics_log[0]
    assert list(a) == list(b) == ["epoch", "train", "test", "test_batches"]
    assert json.dumps(a, sort_keys=True) == json.dumps(b, sort_keys=True)
    assert all(getattr(off, attr) is None for attr in RESULTS.values())


def test_results_are_reset_only_while_their_flag_is_on(log):
    tr = _trainer(True)
    _run(tr)
    kept = {attr: getattr(tr, attr) for attr in RESULTS.values()}
    for f in FLAGS:
        setattr(tr, f, False)
    dl, tl = _loaders()
    tr._train_epoch(dl, tl, epoch=1)
    assert list(tr.metrics_log[1]) == ["epoch", "train", "test", "test_batches"]
    assert all(getattr(tr, attr) is kept[attr] for attr in kept)           # the last logged epoch's results stay
    tr.log_fss = True
    tr._train_epoch(dl, tl, epoch=2)
    assert list(tr.metrics_log[2]) == ["epoch", "train", "test", "test_batches", "fss"]
    assert tr.fss_results is not kept["fss_results"] and set(tr.fss_results) == {"train", "test"}
    assert all(getattr(tr, attr) is kept[attr] for attr in kept if attr != "fss_results")


def test_importing_the_trainer_imports_no_diagnostic_module():
    """In a fresh interpreter: this module itself imports them all."""
    code = ("import sys, downgan_amd.GAN.wasserstein\n"
            "print(sorted(m for m in sys.modules if m.startswith('downgan_amd.') and m.split('.')[1] in %r))" % (
                tuple(mod.__name__.split(".")[1] for mod, _ in STUBBED),))
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", code], cwd=root, check=True, capture_output=True, text=True).stdout
    assert out.strip() == "[]"


def test_an_unknown_keyword_is_a_type_error(log):
    tr = _trainer(None)
    dl, _ = _loaders()
    coarse, fine = next(iter(dl))[:2]
    with pytest.raises(TypeError, match="histmaps"):
        tr.gen_batch_and_log_metrics(coarse, fine, histmaps=object())
    m = tr.gen_batch_and_log_metrics(coarse, fine, fss=None)              # None: not given
    assert set(m) == {"MAE", "MSE", "Wass", "MSSSIM"} and log.passes[-1]["kw"].get("fss") is None and log.passes[-1]["adds"] == []
    xc, xf = tr._stage
    with pytest.raises(TypeError, match="histmaps"):
        tr._engine.metrics_pass(xc, xf, histmaps=object())
