"""A plain reference for the MvNormal log-posteriors, held to a 50-digit sum and then the CPU oracle held to it -- before any GPU
is involved.

The oracle's MvNormal-full likelihood is the device's own form (whitened rows z_i = L^-1 x_i once, then sum_i |z_i - L^-1 mu|^2,
oracle/demc_oracle.c, model_loglike): a mistake in that form would be shared.  `mvn_logpost_ref` is the definition instead,

    sum_i logpdf(MvNormal(mu, Sigma), x_i)  +  sum_j logpdf(prior_j, theta_j),

one observation at a time from the raw data: the residual x_i - mu, one forward substitution with the Cholesky factor of Sigma per
residual, no centring, no whitened copy of the data, no constant pulled out of the sum -- in `np.longdouble` (64-bit significand
on x86).  tests/test_gpu_direct_rows.py compares the DIRECT kernels with it."""
import numpy as np
import pytest

from conftest import make_problem, setup_engine

LD = np.longdouble

# (family, d) of tests/test_gpu_direct_rows.py's log-posterior table
ROWS_TABLE = [("mvn_full", d) for d in (1, 5, 8, 9, 13, 16, 17, 32, 33, 40, 64)] + [("mvn_iso", d) for d in (6, 12, 48)]


def _cholesky_ld(S):
    """lower Cholesky factor in longdouble (numpy.linalg has no longdouble): the textbook column loop"""
    d = S.shape[0]
    L = np.zeros((d, d), LD)
    for j in range(d):
        s = S[j, j]
        for k in range(j):
            s = s - L[j, k] * L[j, k]
        assert s > 0, "Sigma is not positive definite"
        L[j, j] = np.sqrt(s)
        for i in range(j + 1, d):
            s = S[i, j]
            for k in range(j):
                s = s - L[i, k] * L[j, k]
            L[i, j] = s / L[j, j]
    return L


def _log_priors_ld(prob, th):
    """make_problem's prior table on its MvNormal families: kind 1 = Normal(a, b), kind 2 = truncated(Cauchy(a, b), 0, Inf)"""
    pi = 4 * np.arctan(LD(1))
    out = np.zeros(th.shape[0], LD)
    for j, (kind, a, b) in enumerate(zip(prob["pk"], prob["pa"], prob["pb"])):
        a, b, x = LD(a), LD(b), th[:, j]
        z = (x - a) / b
        if kind == 1:
            out += -np.log(2 * pi) / 2 - np.log(b) - z * z / 2
        elif kind == 2:
            mass = 1 - (np.arctan(-a / b) / pi + LD(1) / 2)  # 1 - cdf(0)
            out += np.where(x < 0, -np.inf, -np.log(pi) - np.log(b) - np.log1p(z * z) - np.log(mass))
        else:
            raise KeyError(kind)
    return out


def mvn_logpost_ref(prob, theta):
    """log-posterior of every row of theta under make_problem("mvn_full" | "mvn_iso"), by the definition, in longdouble"""
    from demc_amd import families as F
    X = np.asarray(prob["data"], LD)
    N, d = X.shape
    th = np.asarray(theta, LD).reshape(-1, prob["D"])
    pi = 4 * np.arctan(LD(1))
    R = X[None, :, :] - th[:, None, :d]  # residuals x_i - mu, [row][observation][dimension]
    if prob["fam"] == F.FAM_MVN_FULL:
        L = _cholesky_ld(np.asarray(prob["hyper"], LD).reshape(d, d))
        logdet = 2 * np.log(np.diag(L)).sum()
        Y = np.zeros_like(R)  # L y = r by forward substitution, all residuals at once
        for j in range(d):
            Y[..., j] = (R[..., j] - Y[..., :j] @ L[j, :j]) / L[j, j]
        per_obs = -(d * np.log(2 * pi) + logdet + (Y * Y).sum(-1)) / 2
    elif prob["fam"] == F.FAM_MVN_ISO:
        sg = th[:, d][:, None]  # Sigma = sigma^2 I
        per_obs = -(d * np.log(2 * pi) + 2 * d * np.log(sg) + (R * R).sum(-1) / (sg * sg)) / 2
    else:
        raise KeyError(prob["fam"])
    return per_obs.sum(-1) + _log_priors_ld(prob, th)


def _mp_logpost(prob, theta):
    """the same sum restated in mpmath at 50 digits, by another route: Sigma^-1 and det(Sigma) from mpmath's LU, the quadratic
    form r' Sigma^-1 r written out"""
    import mpmath as mp
    from demc_amd import families as F
    X = np.asarray(prob["data"], float)
    N, d = X.shape
    out = []
    for row in np.asarray(theta, float).reshape(-1, prob["D"]):
        t = [mp.mpf(float(v)) for v in row]
        if prob["fam"] == F.FAM_MVN_FULL:
            S = mp.matrix(np.asarray(prob["hyper"], float).reshape(d, d).tolist())
        else:
            S = mp.eye(d) * t[d] ** 2
        Sinv, logdet = mp.inverse(S), mp.log(mp.det(S))
        ll = mp.mpf(0)
        for i in range(N):
            r = mp.matrix([mp.mpf(float(X[i, k])) - t[k] for k in range(d)])
            ll += -(d * mp.log(2 * mp.pi) + logdet + (r.T * Sinv * r)[0]) / 2
        for j, (kind, a, b) in enumerate(zip(prob["pk"], prob["pa"], prob["pb"])):
            a, b = mp.mpf(float(a)), mp.mpf(float(b))
            z = (t[j] - a) / b
            if kind == 1:
                ll += -mp.log(2 * mp.pi) / 2 - mp.log(b) - z * z / 2
            else:
                ll += -mp.log(mp.pi) - mp.log(b) - mp.log(1 + z * z) - mp.log(1 - (mp.atan(-a / b) / mp.pi + mp.mpf(1) / 2))
        out.append(ll)
    return out


@pytest.mark.parametrize("family", ["mvn_full", "mvn_iso"])
def test_plain_reference_against_a_50_digit_sum(family):
    """1e-17 relative: what the 64-bit significand of longdouble (2^-64 = 5.4e-20 a rounding) leaves of a sum of 40 terms of one
    sign, each behind a d = 5 substitution"""
    mp = pytest.importorskip("mpmath")
    if np.finfo(LD).nmant < 63:
        pytest.skip("np.longdouble has no 64-bit significand on this platform")
    mp.mp.dps = 50
    prob = make_problem(family, np.random.default_rng(4001), N=40, d=5)
    th = prob["init"](4)
    got, want = mvn_logpost_ref(prob, th), _mp_logpost(prob, th)

    def exact(g):  # a longdouble is the sum of two doubles: its leading 53 bits and the rest
        hi = float(g)
        return mp.mpf(hi) + mp.mpf(float(g - LD(hi)))

    worst = float(max(abs((exact(g) - w) / w) for g, w in zip(got, want)))
    print(f"\n{family}: mvn_logpost_ref vs the 50-digit sum, largest relative difference {worst:.2e}")
    assert worst < 1e-17


_ORACLE_CASES = [(f, d, 129) for f, d in ROWS_TABLE] + [("mvn_full", 64, 700)]
_worst = {}


@pytest.mark.parametrize("family,d,N", _ORACLE_CASES)
def test_oracle_against_the_plain_reference(orc, family, d, N):
    """1e-13 relative.  Against a 50-digit sum the oracle's own largest relative error was 7.9e-16 (d in {5, 16, 40, 64}, N in
    {130, 700}, Sigma of condition number under 10): the bar leaves two orders over what the oracle's double arithmetic does."""
    prob = make_problem(family, np.random.default_rng(4100 + 7 * d + N), N=N, d=d)
    th = prob["init"](12)
    o = orc.Oracle(n_groups=2, Np=6, D=prob["D"], schedule=1)
    setup_engine(o, prob)
    got = o.logpost(th)
    o.close()
    want = mvn_logpost_ref(prob, th)
    assert np.isfinite(got).all()
    rel = float(np.max(np.abs((got.astype(LD) - want) / want)))
    _worst[(family, d, N)] = rel
    print(f"\n{family} d={d} N={N}: oracle vs mvn_logpost_ref, largest relative difference {rel:.2e}"
          f"   (largest so far, all cases: {max(_worst.values()):.2e})")
    assert rel < 1e-13


def test_plain_reference_sees_what_the_shortcuts_could_hide():
    """the reference is the definition, so it must move with each ingredient: an observation dropped, an off-diagonal of Sigma
    ignored, a prior left out all change it by far more than the bars above"""
    prob = make_problem("mvn_full", np.random.default_rng(4200), N=40, d=5)
    th = prob["init"](3)
    base = mvn_logpost_ref(prob, th)
    short = dict(prob, data=prob["data"][:-1])
    diag = dict(prob, hyper=np.diag(np.diag(prob["hyper"])))
    flat = dict(prob, pb=[2.0] * 5)
    for other in (short, diag, flat):
        assert np.all(np.abs((mvn_logpost_ref(other, th) - base) / base) > 1e-6)
    # and it is the textbook value where that is known in closed form: d = 1, one observation, Sigma = 4, mu = 0, x = 2
    one = dict(prob, data=np.array([[2.0]]), hyper=np.array([[4.0]]), D=1, pk=[1], pa=[0.0], pb=[1.0])
    want = -0.5 * np.log(2 * np.pi * 4.0) - 0.5 - 0.5 * np.log(2 * np.pi)
    assert abs(float(mvn_logpost_ref(one, np.zeros((1, 1)))[0]) - want) < 1e-15
