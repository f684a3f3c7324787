"""Weight schedules of the weighted synchronous solver (scopa_cfr_sync_iterate_weighted): CFR+, Linear CFR and Discounted CFR.

After iteration t's increments the kernel multiplies every touched cell: a positive regret by pos_t, any other regret by neg_t, the strategy sum by
strat_t.  The library takes these three numbers per iteration as data and computes none of them; they are made here, in float64 numpy:

    vanilla                 1                 1                 1
    cfr+                    1                 0                 t / (t + 1)          regret-matching+ with linear averaging (Tammelin 2014)
    linear                  t / (t + 1)       t / (t + 1)       t / (t + 1)          Brown & Sandholm 2019, = dcfr(1, 1, 1)
    dcfr(alpha, beta, gamma) t^a / (t^a + 1)  t^b / (t^b + 1)   (t / (t + 1))^gamma  Brown & Sandholm 2019; their recommended (1.5, 0, 2)

Scaling a whole table does not change regret matching or the average policy, so multiplying by t / (t + 1) after iteration t is weighting
iteration t's increment by t (up to a common factor).
"""
import numpy as np

VARIANTS = ("vanilla", "cfr+", "linear", "dcfr")


def _discount(t, exponent):
    """t^e / (t^e + 1); e = -inf gives 0 (t = 1 included: the limit taken over t > 1), e = +inf gives 1"""
    if exponent == -np.inf:
        return np.zeros_like(t)
    if exponent == np.inf:
        return np.ones_like(t)
    with np.errstate(over="ignore", invalid="ignore"):
        p = t ** float(exponent)
        return np.where(np.isinf(p), 1.0, p / (p + 1.0))


def schedule(variant, t0, n, alpha=1.5, beta=0.0, gamma=2.0):
    """-> float64 [n][3], rows (pos_t, neg_t, strat_t) for t = t0 + 1 .. t0 + n; every value lies in [0, 1]."""
    if variant not in VARIANTS:
        raise ValueError(f"variant must be one of {VARIANTS}")
    if t0 < 0 or n < 0:
        raise ValueError("t0 and n must be >= 0")
    if np.isnan([alpha, beta, gamma]).any() or gamma < 0:
        raise ValueError("alpha, beta must not be NaN and gamma must be >= 0")
    t = np.arange(int(t0) + 1, int(t0) + int(n) + 1, dtype=np.float64)
    w = np.ones((t.size, 3))
    if variant == "cfr+":
        w[:, 1] = 0.0
        w[:, 2] = t / (t + 1.0)
    elif variant == "linear":
        alpha, beta, gamma = 1.0, 1.0, 1.0
    if variant in ("linear", "dcfr"):
        w[:, 0] = _discount(t, alpha)
        w[:, 1] = _discount(t, beta)
        w[:, 2] = (t / (t + 1.0)) ** float(gamma)
    return w
