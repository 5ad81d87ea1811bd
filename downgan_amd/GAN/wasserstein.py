"""Drop-in mirror of the reference trainer (reference DoWnGAN/GAN/wasserstein.py:16-189).

``WassersteinGAN(G, C, G_optimizer, C_optimizer)`` with the same method names and argument meaning.
Differences, all additive: the iteration methods RETURN the scalars the reference computes and drops
(:46-50, :74-78); ``alpha`` can be injected into ``_critic_train_iteration`` / ``_gp`` (the reference
draws it from the device RNG at :91); Adam is the fused native kernel; when ``torch.optim.Adam`` objects
built the reference's way (stage.py:63-64 over ``G.parameters()`` / ``C.parameters()``) are passed, their lr / betas /
eps are adopted, otherwise ``config.hyperparams`` applies (the arguments may be None).  The epoch loop keeps the reference's per-batch metrics pass, test-set pass, epoch means and per-epoch checkpoints
(:138-179) with mlflow / plotting replaced by return values, ``metrics_log`` and plain files.
"""
from __future__ import annotations

import os
from typing import Callable, NamedTuple, Optional

import torch

from ..config import hyperparams as hp
from ..engine import METRIC_SINKS, TrainEngine
from .. import backend


def _adam_config(opt, base):
    """Hyper-parameters of a ``torch.optim.Adam`` built the reference's way (stage.py:63-64) -> engine HyperParams.  The
    optimizer object itself never steps: Adam runs as the fused native kernel over the flat parameter buffers."""
    if opt is None or not hasattr(opt, "param_groups"):
        return base
    import dataclasses
    g = opt.param_groups[0]
    if type(opt).__name__ != "Adam" or g.get("weight_decay", 0) or g.get("amsgrad", False) or g.get("maximize", False):
        raise NotImplementedError("the native trainer implements plain Adam (no weight decay / amsgrad), as the reference configures it")
    return dataclasses.replace(base, lr=float(g["lr"]), beta1=float(g["betas"][0]), beta2=float(g["betas"][1]), eps=float(g["eps"]))


class WassersteinGAN:
    def __init__(self, G, C, G_optimizer=None, C_optimizer=None, dist=None) -> None:
        self.G, self.C = G, C
        self.G_optimizer, self.C_optimizer = G_optimizer, C_optimizer
        self.num_steps = 0
        self.dist = dist
        self._engine = None
        self._stage = None
        self.last = {}
        self.metrics_log = []

    engine_class = TrainEngine   # the native engine _build creates (WassersteinGANFS: TrainEngineFS)
    check_finite = False         # debug: NaN / Inf census after every iteration (TrainEngine(check_finite=True); the reference
                                 # runs with torch.autograd.set_detect_anomaly(True), wasserstein.py:13)

    def _eng(self, coarse, fine):
        """The shape-bound native engine for this batch.  A batch of another size (a DataLoader's ragged last batch, a test loader
        with its own batch size) re-creates it; the master parameters AND both Adam states (m, v, step count) are carried over on
        the device, so training continues exactly as with one optimizer (stage.py:63-64 builds them once).  The old engine's
        buffers are released BEFORE the new ones are allocated (cfg2: 142 GiB each)."""
        B, cin, S, _ = coarse.shape
        if self._engine is None or (self._engine.B, self._engine.S) != (B, S):
            assert self.G.dtype == self.C.dtype
            carry = old_shape = None
            if self._engine is not None and self._engine.S == S:
                old = self._engine
                old_shape = (old.B, tuple(self._stage[1].shape[1:3]))
                carry = (old.G.P.export_state(), old.C.P.export_state())      # flat fp32 buffers only (8.8 GB at cfg2)
                self.G._bound = self.C._bound = None                          # (no host round trip: the state moves on the device)
                self._engine = self._stage = old = None
                import gc
                gc.collect()
                if torch.cuda.is_available():
                    torch.cuda.empty_cache()
            try:
                e = self._build(B, cin, S, carry)
            except Exception:
                # The live parameters and Adam state exist only in ``carry`` now (the old engine was released to make room).  Put
                # them back into an engine of the size that was running, so that state_dict() / checkpoints / the next batch see
                # the trained weights and not the networks' stale host copies; then let the caller see the failure.
                if carry is not None and old_shape is not None:
                    import gc
                    gc.collect()
                    if torch.cuda.is_available():
                        torch.cuda.empty_cache()
                    self._install(self._build(old_shape[0], cin, S, carry), old_shape[1])
                raise
            self._install(e, (fine.shape[2], fine.shape[3]))
        return self._engine

    def _build(self, B, cin, S, carry):
        ops = backend.make_ops(self.G.dtype, self.G.device)
        e = self.engine_class(ops, S, self.G.filters, cin, B, hp.as_engine_hp(B), self.G.n_predictands,
                              self.G.num_res_blocks, self.G.num_upsample, dist=self.dist, check_finite=self.check_finite)
        if carry is not None:
            e.G.P.import_state(carry[0]); e.C.P.import_state(carry[1])
        return e, carry is not None

    def _install(self, built, fine_hw):
        e, carried = built
        self.G.bind(e.G, load=not carried)
        self.C.bind(e.C, load=not carried)
        self._adopt_optimizers(e)
        e.num_steps = self.num_steps
        self._engine = e
        self._stage = (e.ops.zeros(e.B, e.S, e.S, e.G.cin_p), e.ops.zeros(e.B, fine_hw[0], fine_hw[1], e.G.np_p))

    def _adopt_optimizers(self, e):
        e.adam_hp[id(e.G.P)] = _adam_config(self.G_optimizer, e.hp)
        e.adam_hp[id(e.C.P)] = _adam_config(self.C_optimizer, e.hp)

    def _to_native(self, e, coarse, fine):
        o = e.ops
        if hasattr(coarse, "nhwc"):            # dataloader.NativeBatch: already in native layout (ResidentLoader)
            return coarse.nhwc, fine.nhwc
        xc, xf = self._stage
        o.nchw_to_nhwc(coarse.to(device=o.device, dtype=torch.float32).contiguous(), xc)
        o.nchw_to_nhwc(fine.to(device=o.device, dtype=torch.float32).contiguous(), xf)
        return xc, xf

    def _alpha(self, e, alpha):
        if alpha is None:
            return torch.rand(e.B, device=e.ops.device, dtype=torch.float32)     # wasserstein.py:91
        return torch.as_tensor(alpha, dtype=torch.float32).reshape(-1).to(e.ops.device)

    def _critic_train_iteration(self, coarse, fine, alpha=None, _keep_g=False):
        """``_keep_g`` (set by ``_train_epoch`` on generator steps): keep G(coarse) of this iteration for the generator
        iteration that follows on the same batch, which then skips its own identical forward."""
        e = self._eng(coarse, fine)
        xc, xf = self._to_native(e, coarse, fine)
        e.critic_iteration(xc, xf, self._alpha(e, alpha), save_g=_keep_g)
        self.last = e.read_scalars(False)
        return self.last

    def _generator_train_iteration(self, coarse, fine, _reuse_g=False):
        e = self._eng(coarse, fine)
        xc, xf = self._to_native(e, coarse, fine)
        e.generator_iteration(xc, xf, reuse_fake=_reuse_g)
        out = e.read_scalars(True)
        self.last.update({k: out[k] for k in ("g_loss", "content_loss", "g_c_fake_mean")})
        return {k: out[k] for k in ("g_loss", "content_loss", "g_c_fake_mean")}

    def _gp(self, real, fake, critic=None, alpha=None):
        """Value of gp_lambda * mean((||grad||-1)^2) (wasserstein.py:87-117) for NCHW real / fake."""
        B = real.shape[0]
        e = self._engine
        assert e is not None and e.B == B, "call a train iteration first (buffers are shape-bound)"
        o = e.ops
        xr = o.zeros(*e.fine_shape); o.nchw_to_nhwc(real.to(o.device, torch.float32).contiguous(), xr)
        xk = o.zeros(*e.fine_shape); o.nchw_to_nhwc(fake.to(o.device, torch.float32).contiguous(), xk)
        o.gp_interp(xr, xk, self._alpha(e, alpha), e.xhat)
        e.C.forward(e.xhat)
        e.C.backward(e.xhat, 1.0, wgrad=False, dx=e.gbuf)
        e.ss.zero_()
        o.sumsq_rows(e.gbuf, e.ss)
        o.gp_finish(e.ss, B, B * e.world, e.hp.gp_lambda, 0.0, e.coef, e._sc("gp_ret"))
        return float(e._sc("gp_ret").item())

    def gen_batch_and_log_metrics(self, coarse, fine, spectra=None, distributions=None, maps=None, fss=None, joint=None,
                                  coherence=None, increments=None, hist_maps=None, temporal=None, helmholtz=None, objects=None,
                                  distances=None, intensity_scale=None):
        """Native version of mlflow_tools/mlflow_epoch.py:53-63 (the per-step metrics pass, wasserstein.py:140):
        returns {"MAE", "MSE", "Wass", "MSSSIM"} (MSSSIM None for tiles too small for 5 scales).  The other keywords are the
        diagnostic sinks of ``TrainEngine.metrics_pass`` (engine.METRIC_SINKS), accumulators that also receive the real and
        generated fields of this batch; only those given (not None) are handed to the engine."""
        given = locals()                                      # the arguments by name, before any other local exists
        sinks = {name: given[name] for name, _ in METRIC_SINKS if given[name] is not None}
        e, n = self._engine, coarse.shape[0]
        if (e is not None and n < e.B and coarse.shape[2] == e.S and not hasattr(coarse, "nhwc")
                and (e.dist is None or e.world == 1)):
            # a smaller batch (a test loader's own batch size, a ragged last batch) on the TRAINING engine's buffers, padded:
            # re-binding would tear down and re-allocate every training buffer (142 GiB at configs[1]) for one G forward and two
            # critic forwards, and once more when the next training batch arrives.  Larger batches still re-bind (the MS-SSIM
            # normalisation runs over the whole batch, losses.py:15-29, so they cannot be split).
            o = e.ops
            xc, xf = self._stage
            o.nchw_to_nhwc(coarse.to(device=o.device, dtype=torch.float32).contiguous(), xc[:n])
            o.nchw_to_nhwc(fine.to(device=o.device, dtype=torch.float32).contiguous(), xf[:n])
        else:
            e, n = self._eng(coarse, fine), None              # the whole batch counts
            xc, xf = self._to_native(e, coarse, fine)
        return e.metrics_pass(xc, xf, n_valid=n, **sinks)

    # what the reference's epoch loop does beside the two iterations (wasserstein.py:138-179), switchable because it costs one
    # extra G forward + two critic forwards per batch: the per-batch metrics pass on the train set, the same pass over the test
    # set at the epoch's end, per-epoch means (post_epoch_metric_mean), and the per-epoch checkpoint of both networks
    log_metrics = True
    # opt-in: radially averaged power spectra of the real and generated fields of the metrics passes (train batches, test
    # loader), accumulated on the device and reported per epoch in summary["spectra"]; rides on the metrics pass's G forward
    log_spectra = False
    # opt-in: value histograms of the same real and generated fields (quantiles, W1 / KS distances, tail exceedances), reported
    # per epoch in summary["distributions"]; distribution_spec None = histograms.HistSpec.zscore(n_predictands)
    log_distributions = False
    distribution_spec = None
    distribution_q = (0.001, 0.01, 0.05, 0.25, 0.5, 0.75, 0.95, 0.99, 0.999)
    distribution_exceed_q = (0.99, 0.999, 0.9999)
    distribution_results = None  # the last epoch's {"train" / "test": (real, fake) histograms.Histogram} when logged
    # opt-in: per-gridpoint statistics maps of the same real and generated fields (mean, std, skewness, extremes, exceedance
    # frequencies, bias / MAE / RMSE / temporal correlation), their summary reported per epoch in summary["maps"]; map_spec None
    # = gridstats.GridSpec.zscore(n_predictands); map_dir: the maps are saved under <map_dir>/<epoch>/<part>/ as .npy files
    log_maps = False
    map_spec = None
    map_dir = None
    map_results = None           # the last epoch's {"train" / "test": gridstats.GridMaps} when logged
    # opt-in: the fractions skill score of the same (real, generated) pairs per threshold and neighbourhood size (exact integer
    # sums on the device), its summary reported per epoch in summary["fss"]; fss_spec None = fss.FssSpec.zscore(n_predictands)
    log_fss = False
    fss_spec = None
    fss_results = None           # the last epoch's {"train" / "test": fss.FssResult} when logged
    # opt-in: joint histograms of the same (real, generated) pairs -- wind roses, (u, v) densities and real-vs-generated densities
    # (exact integer tables on the device), their summary reported per epoch in summary["joint"]; joint_spec None =
    # joint.JointSpec.zscore(n_predictands)
    log_joint = False
    joint_spec = None
    joint_results = None         # the last epoch's {"train" / "test": joint.Joint} when logged
    # opt-in: cross spectra of the same (real, generated) pairs -- per-scale coherence, relative error spectrum and the effective
    # resolution (the last wavenumber down to which the coherence stays >= coherence_threshold), reported per epoch in
    # summary["coherence"]
    log_coherence = False
    coherence_threshold = 0.5
    # opt-in: increment histograms of the same (real, generated) pairs -- structure functions, flatness and skewness per
    # separation and direction, W1 / KS distances of the increment distributions (exact integer tables on the device), their
    # summary reported per epoch in summary["increments"]; increment_spec None = increments.IncrementSpec.zscore(n_predictands)
    log_increments = False
    increment_spec = None
    increment_results = None     # the last epoch's {"train" / "test": increments.IncrementResult} when logged
    # opt-in: per-gridpoint histograms of the same (real, generated) pairs -- maps of the local quantiles (quantile_map_q), their
    # bias and the local W1 / KS distances (an exact int32 table per pixel on the device: gridhist.GridHist.nbytes), their summary
    # reported per epoch in summary["quantile_maps"]; quantile_map_spec None = histograms.HistSpec.zscore(n_predictands, bins=64,
    # lim=6.0); quantile_map_dir: the maps are saved under <quantile_map_dir>/<epoch>/<part>/ as .npy files
    log_quantile_maps = False
    quantile_map_spec = None
    quantile_map_q = (0.5, 0.95, 0.99)
    quantile_map_dir = None
    quantile_map_results = None  # the last epoch's {"train" / "test": gridhist.GridHistMaps} when logged
    # opt-in: temporal diagnostics of the (real, generated) pairs of the TEST part only -- spell durations per threshold, ramp
    # histograms per lead time and lag-autocorrelation maps, real against generated (what shows a generator that flickers from
    # frame to frame), reported per epoch in summary["temporal"]; temporal_spec None = temporal.TemporalSpec.zscore(n_predictands);
    # temporal_dir: saved under <temporal_dir>/<epoch>/test/.  The test loader MUST iterate in time order without shuffling: its
    # batches are taken as consecutive times of one series.  Not available under data parallelism (the ranks hold interleaved
    # samples, and a time series cannot be summed over them): world > 1 raises ValueError at the start of the epoch.
    log_temporal = False
    temporal_spec = None
    temporal_dir = None
    temporal_results = None      # the last epoch's {"test": temporal.TemporalResult} when logged
    # opt-in: Helmholtz spectra of the same (real, generated) pairs -- the kinetic energy spectrum of the wind (channels
    # helmholtz_pair = (u, v)) split into its rotational and divergent parts, the divergent fraction per scale and the coherence
    # and effective resolution (at helmholtz_threshold) of each part, reported per epoch in summary["helmholtz"].  helmholtz_scale
    # (su, sv): on z-scored channels pass their standard deviations, the split is not invariant under per-channel scaling;
    # helmholtz_rows_up False: the rows run north to south.  Needs n_predictands >= 2 (ValueError at the start of the epoch)
    log_helmholtz = False
    helmholtz_pair = (0, 1)
    helmholtz_scale = None
    helmholtz_rows_up = True
    helmholtz_threshold = 0.5
    # opt-in: object-based verification of the same (real, generated) pairs -- the connected exceedance objects per threshold
    # (counts, area and mass distributions, per-object POD / FAR / CSI, the SAL score), reported per epoch in summary["objects"];
    # objects_spec None = objects.ObjectSpec.zscore(n_predictands).  Every metrics pass then waits once for its object count
    log_objects = False
    objects_spec = None
    objects_results = None       # the last epoch's {"train" / "test": objects.ObjectsResult} when logged
    # opt-in: distance-map verification of the same (real, generated) pairs -- the exact distance transforms of the exceedance
    # masks per threshold (mean error distance in both directions, Hausdorff distance, Baddeley's Delta, displacement quantiles),
    # reported per epoch in summary["distances"]; distance_spec None = distmap.DistSpec.zscore(n_predictands).  Every metrics
    # pass then waits once for its records
    log_distances = False
    distance_spec = None
    distance_results = None      # the last epoch's {"train" / "test": distmap.DistanceResult} when logged
    # opt-in: intensity-scale verification of the same (real, generated) pairs -- the error of the thresholded fields split into
    # 2-D Haar components per dyadic scale (skill, MSE and energies per threshold and scale; exact integer sums on the device,
    # nothing per pixel), reported per epoch in summary["intensity_scale"]; intensity_scale_spec None =
    # iscale.IscaleSpec.zscore(n_predictands)
    log_intensity_scale = False
    intensity_scale_spec = None
    intensity_scale_results = None   # the last epoch's {"train" / "test": iscale.IscaleResult} when logged
    checkpoint_dir = None        # e.g. "artifacts": <dir>/Critic/Critic_<epoch>/state_dict.pth (mlflow_epoch.py:65-69 without mlflow)

    @staticmethod
    def _metric_means(rows):
        keys = [k for k in ("MAE", "MSE", "MSSSIM", "Wass") if rows and rows[0].get(k) is not None]
        return {k: sum(r[k] for r in rows) / len(rows) for k in keys}

    # ---- the factories of the HOOKS table below the class: (a fine batch [.., H, W], device) -> one part's accumulator(s)
    def _spec(self, spec, cls, **kw):
        """``spec``, or the spec class's z-score default for this generator's channels when it is None."""
        return spec if spec is not None else cls.zscore(self.G.n_predictands, **kw)

    def _spectra_pair(self, fine, dev):
        from ..spectra import RadialSpectrum
        C, N = self.G.n_predictands, fine.shape[-1]
        return RadialSpectrum(C, N, device=dev), RadialSpectrum(C, N, device=dev)

    def _dist_pair(self, fine, dev):
        from ..histograms import HistSpec, ValueHistogram
        spec = self._spec(self.distribution_spec, HistSpec)
        return ValueHistogram(spec, device=dev), ValueHistogram(spec, device=dev)

    def _map_stats(self, fine, dev):
        from ..gridstats import GridSpec, GridStats
        return GridStats(self._spec(self.map_spec, GridSpec), fine.shape[-2], fine.shape[-1], paired=True, device=dev)

    def _fss_acc(self, fine, dev):
        from ..fss import FractionsSkill, FssSpec
        return FractionsSkill(self._spec(self.fss_spec, FssSpec), fine.shape[-2], fine.shape[-1], device=dev)

    def _joint_acc(self, fine, dev):
        from ..joint import JointSpec, ValueJoint
        return ValueJoint(self._spec(self.joint_spec, JointSpec), device=dev)

    def _coherence_acc(self, fine, dev):
        from ..spectra import CrossSpectrum
        return CrossSpectrum(self.G.n_predictands, fine.shape[-1], device=dev)

    def _increment_acc(self, fine, dev):
        from ..increments import Increments, IncrementSpec
        return Increments(self._spec(self.increment_spec, IncrementSpec), device=dev)

    def _quantile_map_acc(self, fine, dev):
        from ..gridhist import GridHist
        from ..histograms import HistSpec
        spec = self._spec(self.quantile_map_spec, HistSpec, bins=64, lim=6.0)
        return GridHist(spec, fine.shape[-2], fine.shape[-1], paired=True, device=dev)

    def _temporal_acc(self, fine, dev):
        from ..temporal import Temporal, TemporalSpec
        return Temporal(self._spec(self.temporal_spec, TemporalSpec), fine.shape[-2], fine.shape[-1], paired=True, device=dev)

    def _helmholtz_acc(self, fine, dev):
        from ..spectra import HelmholtzSpectrum
        return HelmholtzSpectrum(fine.shape[-1], pair=self.helmholtz_pair, scale=self.helmholtz_scale,
                                 rows_up=self.helmholtz_rows_up, device=dev)

    def _objects_acc(self, fine, dev):
        from ..objects import Objects, ObjectSpec
        return Objects(self._spec(self.objects_spec, ObjectSpec), fine.shape[-2], fine.shape[-1], paired=True, device=dev)

    def _distances_acc(self, fine, dev):
        from ..distmap import Distances, DistSpec
        return Distances(self._spec(self.distance_spec, DistSpec), fine.shape[-2], fine.shape[-1], device=dev)

    def _iscale_acc(self, fine, dev):
        from ..iscale import IntensityScale, IscaleSpec
        return IntensityScale(self._spec(self.intensity_scale_spec, IscaleSpec), fine.shape[-2], fine.shape[-1], device=dev)

    def _hooks(self, acc, part, fine):
        """The keyword arguments of gen_batch_and_log_metrics that feed the enabled per-epoch accumulators of ``part``
        ("train" / "test"), created on first use in ``acc`` = {summary key: {part: accumulator(s)}}; {} when none is on."""
        kw = {}
        for h in HOOKS:
            if getattr(self, h.flag) and part in h.parts:
                accs = acc.setdefault(h.key, {})
                if part not in accs:
                    accs[part] = h.make(self, fine, self._engine.ops.device if self._engine is not None else self.G.device)
                kw[h.sink] = accs[part]
        return kw

    def _helmholtz_summary(self, hook, part, acc, epoch):
        """The eight mean planes by name ([K] each), "div_frac_real", "div_frac_fake" (div / (rot + div), NaN on ring 0),
        "coh_rot", "coh_div": [K], "k_eff_rot", "k_eff_div" (effective resolution of each part at ``helmholtz_threshold``),
        "wavelength_px_rot", "wavelength_px_div" and "fields" of one part's accumulator, summed over the data-parallel ranks
        first."""
        from ..spectra import (HELM_CROSS_PLANES, divergent_fraction, effective_resolution, helmholtz_coherence, wavelength_px)
        s = acc.reduce_(self.dist).mean().cpu().numpy()
        frac, coh = divergent_fraction(s), helmholtz_coherence(s)
        out = {name: s[i].tolist() for i, name in enumerate(HELM_CROSS_PLANES)}
        out.update(div_frac_real=frac[0].tolist(), div_frac_fake=frac[1].tolist(), coh_rot=coh[0].tolist(), coh_div=coh[1].tolist())
        for i, what in enumerate(("rot", "div")):
            k = effective_resolution(coh[i], self.helmholtz_threshold)
            out["k_eff_" + what] = int(k)
            out["wavelength_px_" + what] = float(wavelength_px(k, acc.N))
        out["fields"] = acc.count
        return out

    def _coherence_summary(self, hook, part, acc, epoch):
        """{"real", "fake", "co": [C][K] mean spectra of the real and generated fields and their co-spectrum, "coherence",
        "rel_error": [C][K], "k_eff", "wavelength_px": [C] effective resolution at ``coherence_threshold``, "fields": count} of
        one part's accumulator, summed over the data-parallel ranks first."""
        from ..spectra import coherence, effective_resolution, relative_error_spectrum, wavelength_px
        s = acc.reduce_(self.dist).mean().cpu().numpy()
        coh = coherence(s)
        k_eff = effective_resolution(coh, self.coherence_threshold)
        return {"real": s[:, 0].tolist(), "fake": s[:, 1].tolist(), "co": s[:, 2].tolist(), "coherence": coh.tolist(),
                "rel_error": relative_error_spectrum(s).tolist(), "k_eff": [int(k) for k in k_eff],
                "wavelength_px": [float(w) for w in wavelength_px(k_eff, acc.N)], "fields": acc.count}

    def _result_summary(self, h, part, acc, epoch):
        """The JSON-serialisable summary of one part's accumulator of hook ``h`` (summed over the data-parallel ranks first,
        where ``h.reduce``); its result is kept in the ``h.results`` attribute and, with the ``h.dir`` attribute set, saved
        under <dir>/<epoch>/<part> -- by the first rank where the ranks hold the same reduced result.  ``h.q``: the attribute
        whose quantile levels both ``save`` and ``summary`` take."""
        res = (acc.reduce_(self.dist) if h.reduce else acc).result()
        getattr(self, h.results)[part] = res
        args = () if h.q is None else (tuple(getattr(self, h.q)),)
        directory = None if h.dir is None else getattr(self, h.dir)
        if directory is not None and (not h.reduce or self.dist is None or self.dist.rank == 0):
            res.save(os.path.join(directory, str(epoch), part), *args)
        return res.summary(*args)

    def _distribution_summary(self, hook, part, pair, epoch):
        """The JSON-serialisable summary of an accumulator pair (summed over the data-parallel ranks first): channel names,
        field count, quantiles / moments / extrema / out-of-range and NaN counts of the real and the generated values, and per
        channel their W1 and KS distances and the generated values' exceedance of the real tail quantiles."""
        from ..histograms import exceedance, ks_distance, wasserstein1
        real, fake = (acc.reduce_(self.dist).result() for acc in pair)
        q, eq = list(self.distribution_q), list(self.distribution_exceed_q)
        side = lambda h: {"quantiles": h.quantile(q).tolist(), "mean": h.mean().tolist(), "std": h.std().tolist(),
                          "min": h.min().tolist(), "max": h.max().tolist(), "out_of_range": h.out_of_range().tolist(),
                          "nan": h.nan().tolist()}
        self.distribution_results[part] = (real, fake)
        return {"channels": list(real.spec.names), "fields": real.fields, "q": q, "exceed_q": eq, "real": side(real),
                "fake": side(fake), "w1": wasserstein1(real, fake).tolist(), "ks": ks_distance(real, fake).tolist(),
                "exceed_fake": exceedance(real, fake, eq).tolist()}

    def _spectra_summary(self, hook, part, pair, epoch):
        """{"real", "fake": [C][K] mean spectra, "lsd": [C] log-spectral distance of fake to real, "fields": count} of an
        accumulator pair, summed over the data-parallel ranks first."""
        from ..spectra import log_spectral_distance
        real, fake = (acc.reduce_(self.dist).mean() for acc in pair)
        return {"real": real.cpu().tolist(), "fake": fake.cpu().tolist(),
                "lsd": [float(v) for v in log_spectral_distance(real, fake)], "fields": pair[0].count}

    def _train_epoch(self, dataloader, testdataloader=None, epoch=0):
        """wasserstein.py:120-179: every batch = critic iteration, generator iteration when num_steps % critic_iterations == 0
        (same batch), metrics pass (:140-146); then the epoch means of the train metrics, the metrics over the test loader
        (:157-170) and the checkpoint (:178).  Plotting (gen_grid_images) and mlflow are out of scope; the per-step scalars are
        returned and the epoch summary is appended to ``self.metrics_log``."""
        if self.log_temporal and self.dist is not None and self.dist.world_size > 1:
            raise ValueError("log_temporal needs one rank: under data parallelism the ranks hold interleaved samples of the test "
                             f"series, and a time series cannot be summed over them (world size {self.dist.world_size})")
        if self.log_helmholtz:
            from ..spectra import _helm_pair, _helm_scale
            if self.G.n_predictands < 2:
                raise ValueError(f"log_helmholtz needs a wind field: n_predictands >= 2 (got {self.G.n_predictands})")
            _helm_pair(self.helmholtz_pair, self.G.n_predictands)
            _helm_scale(self.helmholtz_scale, self.helmholtz_rows_up)
        log, train_metrics, test_metrics = [], [], []
        acc = {}                                              # summary key of HOOKS -> {"train" / "test": accumulator(s)}
        for data in dataloader:
            coarse, fine = data[0], data[1]
            gen_step = self.num_steps % hp.critic_iterations == 0                 # :136
            out = dict(self._critic_train_iteration(coarse, fine, _keep_g=gen_step))
            if gen_step:
                out.update(self._generator_train_iteration(coarse, fine, _reuse_g=True))
            hooks = self._hooks(acc, "train", fine)
            if hooks:
                m = self.gen_batch_and_log_metrics(coarse, fine, **hooks)
                if self.log_metrics:
                    train_metrics.append(m)
            elif self.log_metrics:
                train_metrics.append(self.gen_batch_and_log_metrics(coarse, fine))   # :140-146
            self.num_steps += 1
            if self._engine is not None:
                self._engine.num_steps = self.num_steps
            log.append(out)
        summary = {"epoch": epoch}
        if self.log_metrics:
            summary["train"] = self._metric_means(train_metrics)                     # :150
            if testdataloader is not None:
                # :157-168.  EVERY test batch is evaluated, whatever its size (the engine re-binds, state carried over); the
                # reference's epoch mean is the mean over batches (post_epoch_metric_mean), a ragged batch counting as one
                for data in testdataloader:
                    test_metrics.append(self.gen_batch_and_log_metrics(data[0], data[1], **self._hooks(acc, "test", data[1])))
                if not test_metrics:
                    raise ValueError("the test loader yielded no batch: no test metrics for this epoch (wasserstein.py:157-170)")
                summary["test"] = self._metric_means(test_metrics)                   # :170
                summary["test_batches"] = len(test_metrics)
        on = [h for h in HOOKS if getattr(self, h.flag)]
        if on:
            if testdataloader is not None and not self.log_metrics:
                for data in testdataloader:
                    self.gen_batch_and_log_metrics(data[0], data[1], **self._hooks(acc, "test", data[1]))
            for h in on:
                if h.results is not None:
                    setattr(self, h.results, {})
                summary[h.key] = {part: h.summary(self, h, part, a, epoch) for part, a in acc.get(h.key, {}).items()}
        if self.checkpoint_dir is not None:
            from ..checkpoint import log_network_models
            summary["checkpoints"] = log_network_models(self.C, self.G, epoch, self.checkpoint_dir)   # :178
        self.metrics_log.append(summary)
        return log

    def train(self, dataloader, testdataloader=None, epochs=None):
        """wasserstein.py:181-189."""
        self.num_steps = 0
        self.metrics_log = []
        history = []
        for epoch in range(hp.epochs if epochs is None else epochs):
            history.append(self._train_epoch(dataloader, testdataloader, epoch))
        return history


class Hook(NamedTuple):
    """One opt-in per-epoch diagnostic of the trainer.  The trainer's attributes are given by name and read when an epoch
    needs them, so they can be set on the class or on an instance at any time."""
    key: str                                   # of the epoch summary, and of the epoch's accumulators
    flag: str                                  # the attribute that switches it on
    sink: str                                  # the keyword of gen_batch_and_log_metrics / TrainEngine.metrics_pass it feeds
    make: Callable                             # (trainer, fine batch, device) -> one part's accumulator, or (real, fake) pair
    summary: Callable = WassersteinGAN._result_summary     # (trainer, hook, part, accumulator, epoch) -> JSON-serialisable dict
    results: Optional[str] = None              # the attribute that keeps {part: result} of the last logged epoch, if any
    parts: tuple = ("train", "test")           # the parts of the epoch it is fed in
    # what _result_summary reads beside ``results``:
    dir: Optional[str] = None                  # the attribute of the directory the results are saved under (None: never saved)
    q: Optional[str] = None                    # the attribute of the quantile levels that save() and summary() take
    reduce: bool = True                        # whether the accumulator is summed over the data-parallel ranks first


HOOKS = (                                      # in the order of the epoch summary's keys
    Hook("spectra", "log_spectra", "spectra", WassersteinGAN._spectra_pair, WassersteinGAN._spectra_summary),
    Hook("distributions", "log_distributions", "distributions", WassersteinGAN._dist_pair, WassersteinGAN._distribution_summary,
         results="distribution_results"),
    Hook("maps", "log_maps", "maps", WassersteinGAN._map_stats, results="map_results", dir="map_dir"),
    Hook("fss", "log_fss", "fss", WassersteinGAN._fss_acc, results="fss_results"),
    Hook("joint", "log_joint", "joint", WassersteinGAN._joint_acc, results="joint_results"),
    Hook("coherence", "log_coherence", "coherence", WassersteinGAN._coherence_acc, WassersteinGAN._coherence_summary),
    Hook("increments", "log_increments", "increments", WassersteinGAN._increment_acc, results="increment_results"),
    Hook("quantile_maps", "log_quantile_maps", "hist_maps", WassersteinGAN._quantile_map_acc, results="quantile_map_results",
         dir="quantile_map_dir", q="quantile_map_q"),
    # the test part only: the train batches are shuffled samples; one rank (_train_epoch), so there is nothing to reduce
    Hook("temporal", "log_temporal", "temporal", WassersteinGAN._temporal_acc, results="temporal_results", dir="temporal_dir",
         reduce=False, parts=("test",)),
    Hook("helmholtz", "log_helmholtz", "helmholtz", WassersteinGAN._helmholtz_acc, WassersteinGAN._helmholtz_summary),
    Hook("objects", "log_objects", "objects", WassersteinGAN._objects_acc, results="objects_results"),
    Hook("distances", "log_distances", "distances", WassersteinGAN._distances_acc, results="distance_results"),
    Hook("intensity_scale", "log_intensity_scale", "intensity_scale", WassersteinGAN._iscale_acc, results="intensity_scale_results"),
)
