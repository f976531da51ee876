"""Host driver mirroring src/main.jl (sample/_sample/sample_init/bundle_samples) and src/optimize.jl on top of the
C-ABI engine.  The per-iteration work -- step!/pstep! (main.jl:84-107) -- happens inside libdemc_hip.so."""
import numpy as np

from . import _ffi
from .chains import COV_MAX_COLS, Bridge, Chains, Hpd, Loo, RankStats, Summary, Waic, hpd_alphas, series_cov, series_quantiles
from .families import PRIOR_NORMAL_REF, Priors, SimulatedLikelihood, SourceLikelihood
from .structs import (DE, HIPBackend, LOGLIKE_MODES, MCMCThreads, SCHEDULES, DEModel, Particle, maximize)


def _shapes(theta):
    return [np.shape(t) for t in theta]


def _flatten(theta):
    return np.concatenate([np.asarray(t, dtype=np.float64).ravel() for t in theta])


def get_names(model, shapes):
    """utilities.jl:131-149 (Julia's CartesianIndices order: first index fastest, 1-based)."""
    names = []
    for k, shp in zip(model.names, shapes):
        if len(shp) == 0:
            names.append(str(k))
        else:
            for lin in range(int(np.prod(shp))):
                idx = np.unravel_index(lin, shp, order="F")
                names.append(f"{k}[{','.join(str(i + 1) for i in idx)}]")
    return names + ["acceptance", "lp"]


def _flat_layout(model, de, theta0):
    """Flatten nested Theta to D scalars: bounds per top-level parameter, zip-truncated
    (utilities.jl:73-78); blocks as nested Bool arrays (structs.jl:45) -> byte masks."""
    shapes = _shapes(theta0)
    sizes = [int(np.prod(s)) if len(s) else 1 for s in shapes]
    D = int(sum(sizes))
    offs = np.concatenate([[0], np.cumsum(sizes)])
    lo = np.full(D, -np.inf)
    hi = np.full(D, np.inf)
    for i, b in enumerate(de.bounds):
        if i >= len(sizes):
            break
        lo[offs[i]:offs[i + 1]] = float(b[0])
        hi[offs[i]:offs[i + 1]] = float(b[1])
    kind = np.zeros(D, np.int32)
    a = np.zeros(D)
    b_ = np.ones(D)
    ref = np.zeros(D, np.int32)
    pri = model.prior_loglike
    if isinstance(pri, Priors):
        for i, nm in enumerate(model.names):
            p = pri.by_name.get(nm)
            if p is None:
                continue
            sl = slice(offs[i], offs[i + 1])
            kind[sl], a[sl], b_[sl] = p.kind, p.a, p.b
            if p.kind == PRIOR_NORMAL_REF:
                j = model.names.index(p.ref)
                if sizes[j] != 1:
                    raise _ffi.DemcError(_ffi.EINVAL, "hierarchical scale must be a scalar parameter")
                ref[sl] = offs[j]
    # de.blocks -> byte masks.  Whether blocking is ON is asked per iteration (de.blocking_on(de), main.jl:137,162),
    # see _blocking_schedule(); the masks are built whenever de.blocks holds real blocks.
    masks = None
    if _has_blocks(de.blocks):
        rows = []
        for blk in de.blocks:
            m = np.zeros(D, np.uint8)
            for i, e in enumerate(blk):
                e = np.asarray(e, dtype=bool)
                m[offs[i]:offs[i + 1]] = e.ravel() if e.ndim else e
            rows.append(m)
        masks = np.stack(rows)
    return dict(shapes=shapes, sizes=sizes, offs=offs, D=D, lo=lo, hi=hi, kind=kind, a=a, b=b_, ref=ref, masks=masks)


def _has_blocks(blocks):
    """DE's default is blocks = [false] (structs.jl:99): a placeholder, not a block list"""
    try:
        return len(blocks) > 0 and not isinstance(blocks[0], (bool, np.bool_))
    except TypeError:
        return False


def _blocking_schedule(de, n_iter):
    """de.blocking_on(de) is a user hook evaluated on every iteration with de.iter set (main.jl:34,137,162).  It runs on
    the host; consecutive iterations with the same answer become one engine call.  -> list of (first_iter, count, on)"""
    saved = de.iter
    flags = []
    for it in range(1, n_iter + 1):
        de.iter = it + de.n_initial
        flags.append(bool(de.blocking_on(de)))
    de.iter = saved
    runs = []
    for i, f in enumerate(flags):
        if runs and runs[-1][2] == f:
            runs[-1][1] += 1
        else:
            runs.append([i + 1, 1, f])
    return runs


def engine_config(de, lay, n_iter, backend, n_groups_local=None, group_offset=0, store_history=True, n_initial=None):
    n_initial = de.n_initial if n_initial is None else n_initial
    seed = backend.seed if backend.seed is not None else int(np.random.randint(0, 2**62))
    return dict(n_groups=de.n_groups if n_groups_local is None else n_groups_local, Np=de.Np, D=lay["D"], n_blocks=0,
                burnin=de.burnin, n_initial=n_initial, n_rows=n_iter + n_initial, alpha=de.α, beta=de.β, eps=de.ϵ,
                sigma=de.σ, kappa=de.κ, theta_snooker=de.θsnooker, proposal_kind=de.generate_proposal.code,
                partner_kind=de.sample.code, update_kind=de.update_particle.code,
                fitness_kind=de.evaluate_fitness.code, schedule=SCHEDULES[backend.schedule],
                store_history=1 if store_history else 0, group_offset=group_offset, n_groups_total=de.n_groups,
                seed=seed, device_id=backend.device_id, loglike_mode=LOGLIKE_MODES[backend.loglike_mode])


def configure_engine(eng, model, lay):
    if isinstance(model.loglike, SimulatedLikelihood):  # a simulator, not a density: demc_set_model_sim
        model.loglike.configure(eng, model.data, lay["shapes"])
        eng.set_priors(lay["kind"], lay["a"], lay["b"], lay["ref"])
        eng.set_bounds(lay["lo"], lay["hi"])
        return
    data, dims, hyper = model.loglike.pack(model.data, lay["shapes"])
    if isinstance(model.loglike, SourceLikelihood) and model.loglike.row:
        eng.set_model_source_row(model.loglike.source, data, dims, hyper, has_prior=model.loglike.has_prior)
    elif isinstance(model.loglike, SourceLikelihood):
        eng.set_model_source(model.loglike.source, data, dims, hyper)
    else:
        eng.set_model(model.loglike.family, data, dims, hyper)
    eng.set_priors(lay["kind"], lay["a"], lay["b"], lay["ref"])
    eng.set_bounds(lay["lo"], lay["hi"])


def sample_init(model, de, n_iter, lay, P):
    """main.jl:263-271 + utilities.jl:13-41: history rows 1:n_initial are independent prior draws per particle;
    Theta starts at samples[1,:,id] when n_initial > 0, else at a fresh prior draw.  Ids run 1..P group-major
    in the reference; here 0..P-1."""
    D = lay["D"]
    init_rows = np.empty((de.n_initial, P, D))
    for p in range(P):
        for i in range(de.n_initial):
            init_rows[i, p] = _flatten(model.sample_prior())
    if de.n_initial > 0:
        theta = init_rows[0].copy()
    else:
        theta = np.stack([_flatten(model.sample_prior()) for _ in range(P)])
    return theta, init_rows


def rekey_by_id(th, acc, lp, idh, id0=0, P_total=None):
    """History comes back keyed by slot plus the id that occupied the slot; the reference keys by particle id
    (samples[iter, :, p.id], utilities.jl:170-180; accept/lp live on the Particle object)."""
    n, P, D = th.shape
    P_total = P if P_total is None else P_total
    oth = np.zeros((n, P_total, D))
    oacc = np.zeros((n, P_total), np.uint8)
    olp = np.zeros((n, P_total))
    rows = np.arange(n)[:, None]
    cols = idh - id0
    oth[rows, cols] = th
    oacc[rows, cols] = acc
    olp[rows, cols] = lp
    return oth, oacc, olp


def bundle_samples(model, de, lay, full, n_iter):
    """main.jl:222-250, including its row selection: rows offset+1 .. offset+Ns of the history with
    offset = burnin (or 0), which ignores the n_initial offset.  Deviation (q2): accept/lp are
    paired with Theta by particle id rather than by final slot.  `full` is [rows][D+2][P] by particle id."""
    Ns = n_iter - de.burnin if de.discard_burnin else n_iter
    offset = de.burnin if de.discard_burnin else 0
    names = get_names(model, lay["shapes"])
    return Chains(full[offset:offset + Ns], names, parameters=names[:-2])


def _parse(args):
    backend = None
    rest = []
    for a in args:
        if isinstance(a, (MCMCThreads, HIPBackend)):
            backend = a
        else:
            rest.append(a)
    if len(rest) != 1:
        raise TypeError("sample(model, de, [MCMCThreads()|HIPBackend()], n_iter)")
    if not isinstance(backend, HIPBackend):
        backend = HIPBackend()
    return backend, int(rest[0])


def _run(model, de, n_iter, backend, progress, engine_factory, summary=None):
    if not isinstance(model, DEModel) or not isinstance(de, DE):
        raise TypeError("sample(model::DEModel, de::DE, ...)")
    theta0 = model.sample_prior()
    lay = _flat_layout(model, de, theta0)
    P = de.n_groups * de.Np
    cov_cols = None
    if summary is not None and len(summary) > 4 and summary[4] is not None:  # the series of cor=...: checked before the run
        cov_cols = _cov_cols(get_names(model, lay["shapes"]), summary[4])[1]
    cfg = engine_config(de, lay, n_iter, backend)
    eng = (engine_factory or _ffi.HipEngine)(**cfg)
    want_waic = summary is not None and len(summary) > 5 and summary[5]
    want_loo = summary is not None and len(summary) > 6 and summary[6]
    want_bridge = summary is not None and len(summary) > 7 and summary[7]
    want_rank = summary is not None and len(summary) > 8 and summary[8]
    want_hpd = summary is not None and len(summary) > 9 and summary[9]
    try:
        if want_bridge and not hasattr(eng, "bridge"):  # (no host form: the host route is what the call exists to avoid)
            raise _ffi.DemcError(_ffi.EUNSUPPORTED, "summarize(..., bridge=True) needs an engine with bridge(row0, row1, n_prop, seed) (demc_bridge)")
        if want_loo and not hasattr(eng, "loo"):  # (no host form either: the terms exist on the device only)
            raise _ffi.DemcError(_ffi.EUNSUPPORTED, "summarize(..., loo=True) needs an engine with loo(row0, row1, pointwise): the per-observation "
                                                    "log-densities exist on the device only (demc_loo)")
        if want_waic and not hasattr(eng, "waic"):  # (no host form: the host has no densities)
            raise _ffi.DemcError(_ffi.EUNSUPPORTED, "summarize(..., waic=True) needs an engine with waic(row0, row1, pointwise): the per-observation "
                                                    "log-densities exist on the device only (demc_waic)")
        configure_engine(eng, model, lay)
        if want_waic and hasattr(eng, "waic_served"):  # what demc_waic is certain to refuse is refused before the run, not after it
            eng.waic_served()
        if want_loo and hasattr(eng, "loo_served"):  # likewise demc_loo
            eng.loo_served()
        if want_bridge and hasattr(eng, "bridge_served"):  # likewise demc_bridge
            eng.bridge_served()
        theta, init_rows = sample_init(model, de, n_iter, lay, P)
        if de.n_initial > 0:
            eng.set_history_rows(0, init_rows)
        eng.set_state(theta)  # weights: evaluate_fitness! on device (utilities.jl:19)
        # for iter in 1:n_iter: de.iter = iter + n_initial; groups = stepfun(model, de, groups)  (main.jl:33-38)
        no_blocks = np.zeros((0, lay["D"]), np.uint8)
        done = 0
        for first, count, on in _blocking_schedule(de, n_iter):
            if on and lay["masks"] is None:
                raise _ffi.DemcError(_ffi.EINVAL, "blocking_on(de) is true but de.blocks holds no blocks")
            eng.set_blocks(lay["masks"] if on else no_blocks)
            chunk = max(1, n_iter // 20) if progress else count
            it = first
            while it < first + count:
                n = min(chunk, first + count - it)
                eng.step(it + de.n_initial, n)
                it += n
                done += n
                if progress:
                    print(f"\rDE-MCMC {done}/{n_iter}", end="", flush=True)
        if progress:
            print()
        de.iter = n_iter + de.n_initial
        n_rows = n_iter + de.n_initial
        if want_waic:  # the same kept rows as the other tables, in the same run (demc_waic)
            lay["waic"] = Waic(*eng.waic(summary[0], summary[1], want_waic == "pointwise"))
        if want_loo:  # PSIS-LOO of the same kept rows (demc_loo)
            lay["loo"] = Loo(*eng.loo(summary[0], summary[1], want_loo == "pointwise"))
        if want_bridge:  # the marginal likelihood from the same kept rows (demc_bridge)
            opts = dict(want_bridge) if isinstance(want_bridge, dict) else {}
            lay["bridge"] = Bridge(eng.bridge(summary[0], summary[1], int(opts.get("n_prop", 0)), int(opts.get("seed", 0))))
        if want_rank and hasattr(eng, "rankstats"):  # ess_bulk / ess_tail / rank-normalised rhat of the same kept rows (demc_rankstats)
            lay["rank"] = eng.rankstats(summary[0], summary[1], summary[2])
        if want_hpd and hasattr(eng, "hpd"):  # the highest-density intervals of the same kept rows (demc_hpd)
            lay["hpd"] = eng.hpd(summary[0], summary[1], want_hpd)
        if (summary is not None and (not want_rank or "rank" in lay) and (not want_hpd or "hpd" in lay) and hasattr(eng, "summarize") and (len(summary) < 4 or summary[3] is None or hasattr(eng, "quantiles"))
                and (cov_cols is None or hasattr(eng, "covariance"))):
            # summarize(): the statistics (and the quantiles and the covariance, when asked for) on the device, no export at all
            stats = eng.summarize(summary[0], summary[1], summary[2])[0]
            q = None if len(summary) < 4 or summary[3] is None else eng.quantiles(summary[0], summary[1], summary[3])
            if cov_cols is not None:
                return lay, (stats, q, eng.covariance(summary[0], summary[1], cov_cols)), None
            return lay, (stats if q is None else (stats, q)), None
        if hasattr(eng, "export_chains"):  # device-side re-key + layout (demc_export_chains)
            full = eng.export_chains(0, n_rows)  # [n_rows][D+2][P] by particle id
        else:  # engines without it (the CPU oracle injected by tests): re-key on the host
            th, acc, lp = rekey_by_id(*eng.get_history(0, n_rows))
            full = np.concatenate([np.transpose(th, (0, 2, 1)), acc[:, None, :].astype(np.float64), lp[:, None, :]], axis=1)
        state = eng.get_state()
    finally:
        eng.close()
    return lay, full, state


def sample(model, de, *args, progress=False, engine_factory=None, **kwargs):
    """sample(model, de, n_iter) / sample(model, de, MCMCThreads(), n_iter) (main.jl:19-20, 62-71) and
    sample(model, de, HIPBackend(...), n_iter).  Every form runs on the MI355X; there is no CPU path."""
    backend, n_iter = _parse(args)
    lay, full, _ = _run(model, de, n_iter, backend, progress, engine_factory)
    de.samples = full[:, :lay["D"], :]  # the reference's de.samples: (rows, parameters, particle id)
    return bundle_samples(model, de, lay, full, n_iter)


def _cov_cols(names, cor):
    """cor=True: the parameters; a tuple of names: those series (acceptance and lp may be among them) -> (names, indices)"""
    sel = [nm for nm in names if nm not in ("acceptance", "lp")] if cor is True else list(cor)
    unknown = [nm for nm in sel if nm not in names]
    if unknown or len(set(sel)) != len(sel) or not 1 <= len(sel) <= COV_MAX_COLS:
        raise ValueError(f"cor= takes between 1 and {COV_MAX_COLS} distinct names of {names}" + (f": {unknown} are not among them" if unknown else ""))
    return sel, [names.index(nm) for nm in sel]


def summarize(model, de, *args, max_lag=0, quantiles=None, cor=False, waic=False, loo=False, bridge=False, rank=False, hpd=None, progress=False, engine_factory=None, **kwargs):
    """summarize(model, de, [HIPBackend(...)], n_iter, max_lag=0, quantiles=None, cor=False, waic=False, loo=False, bridge=False, rank=False, hpd=None): the run of sample() followed by the summary
    statistics of the rows bundle_samples keeps (offset = burnin or 0, quirk q1 included) -- computed on the device by
    demc_summarize, so that the history is never exported.  Returns a Summary (chains.py); equal to
    sample(...).summarystats(max_lag) for the same seed.  quantiles: a tuple of probs (chains.DEFAULT_QUANTILES) -- the same run
    also selects those quantiles of the kept rows on the device (demc_quantiles) and the Summary carries them: Summary.quantile()
    equals sample(...).quantile(probs).  cor: True (the parameters) or a tuple of names (acceptance and lp allowed, 64 at most) --
    the same run also forms the covariance and correlation matrices of those series over the kept rows on the device
    (demc_covariance): Summary.cor() / Summary.cov() equal sample(...).cor(names) / .cov(names) to rounding.  An engine without
    summarize, quantiles or covariance (an injected one) exports as sample() does and computes on the host.  waic: True -- the same run
    also forms WAIC over the kept rows on the device (demc_waic) and Summary.waic holds the Waic record; "pointwise"
    keeps the N x 4 table too (what compare_waic reads).  There is no host form of this one: an engine without waic raises
    DemcError(EUNSUPPORTED).  loo: True -- the same run also forms PSIS-LOO over the kept rows on the device (demc_loo) and
    Summary.loo holds the Loo record; "pointwise" keeps the N x 6 table with khat per observation (what compare_loo reads).  A family
    the call cannot serve is refused before the first step, as for waic.  bridge: True or dict(n_prop=, seed=) -- the same run also forms
    the log marginal likelihood over the kept rows on the device by bridge sampling (demc_bridge) and Summary.bridge holds
    the Bridge record (what compare_bridge reads); its rho, the factor se() scales the posterior term by, is taken as kept draws / ESS of lp
    from the same table -- a stated approximation, not a spectral estimate.  rank: True -- the same run also ranks the pooled kept rows
    of every series on the device (demc_rankstats) and Summary.rank holds the RankStats record: ess_bulk, ess_tail and
    the rank-normalised rhat, equal to sample(...).rankstats(max_lag); an engine without rankstats (an injected one) exports as sample()
    does and ranks on the host.  With rank=False the call is what it was.  hpd: an alpha (0.05 for the 95 % interval) or a tuple of
    them -- the same run also reads the highest-density intervals of the pooled kept rows of every series off the sorted pool on the
    device (demc_hpd) and Summary.hpd holds the Hpd record, equal to sample(...).hpd(alphas) bit for bit; an engine
    without hpd (an injected one) exports as sample() does and takes the intervals on the host.  With hpd=None the call is what it was."""
    backend, n_iter = _parse(args)
    Ns = n_iter - de.burnin if de.discard_burnin else n_iter
    offset = de.burnin if de.discard_burnin else 0
    probs = None if quantiles is None else tuple(float(q) for q in quantiles)
    want_cov = None if cor is False or cor is None else (True if cor is True else tuple(cor))
    alphas = None if hpd is None else hpd_alphas(hpd)
    if isinstance(bridge, dict) and set(bridge) - {"n_prop", "seed"}:
        raise ValueError("bridge= takes True or dict(n_prop=, seed=)")
    lay, res, state = _run(model, de, n_iter, backend, progress, engine_factory,
                           summary=(offset, offset + Ns, max_lag, probs, want_cov, waic, loo, True if bridge is True else (dict(bridge) if isinstance(bridge, dict) else bridge), bool(rank), alphas))
    out = _summary_of(model, de, lay, res, state, n_iter, max_lag, probs, want_cov, want_rank=bool(rank) and "rank" not in lay,
                      want_hpd=None if "hpd" in lay else alphas)
    if "hpd" in lay:
        out.hpd = Hpd(out.names, lay["hpd"], alphas)
    if "rank" in lay:
        out.rank = RankStats(out.names, lay["rank"])
    out.waic = lay.get("waic")
    out.loo = lay.get("loo")
    out.bridge = lay.get("bridge")
    if out.bridge is not None:  # the autocorrelation factor of the estimate half: kept draws / ESS of lp, from the table of the same rows
        ess = out["lp"]["ess"]
        kept = Ns * de.n_groups * de.Np
        out.bridge.rho = max(1.0, kept / ess) if np.isfinite(ess) and ess > 0 else 1.0
    return out


def _summary_of(model, de, lay, res, state, n_iter, max_lag, probs, want_cov, want_rank=False, want_hpd=None):
    if state is None:
        names = get_names(model, lay["shapes"])
        if want_cov is not None:
            stats, q, (_, cov, cor_m) = res
            return Summary(names, stats, quantiles=q, probs=probs, cov=cov, cor=cor_m, cov_names=_cov_cols(names, want_cov)[0])
        if probs is None:
            return Summary(names, res)
        return Summary(names, res[0], quantiles=res[1], probs=probs)
    chains = bundle_samples(model, de, lay, res, n_iter)
    out = chains.summarystats(max_lag)
    if want_rank:  # (an engine without rankstats: the definition on the host, from the exported rows)
        out.rank = chains.rankstats(max_lag)
    if want_hpd is not None:  # (an engine without hpd: likewise)
        out.hpd = chains.hpd(want_hpd)
    if probs is not None:
        out.probs = probs
        out.quantiles = np.stack([series_quantiles(chains.value[:, j, :], probs) for j in range(len(chains.names))])
    if want_cov is not None:
        out.cov_names, cols = _cov_cols(chains.names, want_cov)
        _, out.cov_matrix, out.cor_matrix = series_cov(chains.value, cols)
    return out


def optimize(model, de, *args, progress=False, engine_factory=None, **kwargs):
    """optimize(model, de, n_iter) (optimize.jl:17-38): same loop, returns the particles.  n_initial is not
    added to de.iter there (optimize.jl:32, quirk q7); history partners are therefore not supported in this mode."""
    backend, n_iter = _parse(args)
    if de.n_initial != 0:
        raise _ffi.DemcError(_ffi.EUNSUPPORTED, "optimize with n_initial > 0")
    lay, _, (theta, weight, ids) = _run(model, de, n_iter, backend, progress, engine_factory)
    out = []
    for s in range(theta.shape[0]):
        th = [theta[s, lay["offs"][i]:lay["offs"][i + 1]].reshape(shp) if len(shp) else float(theta[s, lay["offs"][i]])
              for i, shp in enumerate(lay["shapes"])]
        out.append(Particle(Θ=th, weight=float(weight[s]), id=int(ids[s])))
    return out


def get_optimal(de, model, particles):
    """utilities.jl:260-266"""
    best = particles[0]
    for p in particles:
        if (p.weight > best.weight) if de.update_particle is maximize else (p.weight < best.weight):
            best = p
    return dict(zip(model.names, best.Θ)), best.weight
