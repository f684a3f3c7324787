"""Helpers of tests/test_gpu_ctx_lifecycle.py: one long-lived context, a mutator, a consumer, and the oracle's answer from scratch.

TEST INFRASTRUCTURE.  The comparisons are the project's own: bit equality (cfr_edges.same_bits) where the kernel is deterministic; for the batched
MCCFR step the per-row reorder budget of tests/test_gpu_mccfr_edges.py (K_REORDER * eps * A_row for one launch, 100 x that over the A_row summed over
several iterations, rtol = atol = 1e-10 for the strategy sums) against oracle.Tree.mccfr_batched; exact equality for visit counters."""
import numpy as np

import mccfr_edges as E

DEALS = {282: 251, 42: 738, 129: 1144, 7: 702}      # py seed -> infosets: set_deal both grows and shrinks every per-deal size
DEFAULT_SEED = 0x5C09A
PAIR = (463, 240)                                   # decision and terminal visits of one traversal pair


def tree(oracle, deal, _cache={}):
    if deal not in _cache:
        _cache[deal] = oracle.Tree(seed=deal)
        assert _cache[deal].n_infosets == DEALS[deal]
    return _cache[deal]


def deal(ctx, sl, oracle, seed):
    t = tree(oracle, seed)
    assert ctx.set_deal(sl.deal_py_seed(seed)) == t.n_infosets
    return t


def restore(ctx, sl):
    """Every mode a case may have touched back to its default.  tests/conftest.py creates a context per test and closes it afterwards, so today this
    guards against nothing that happens; it is kept so that sharing the fixture later stays safe.  It leaves deal 42 set with zero tables -- a fresh
    context has no deal at all, which no entry point can restore."""
    ctx.mccfr_graph_mode(False)
    ctx.sdcfr_mode(0)
    ctx.cfr_exact_mode(False)
    ctx.debug_lds_limit(0)
    ctx.prof_enable(0)
    ctx.p2p_destroy()
    ctx.mccfr_seed(DEFAULT_SEED)
    ctx.set_deal(sl.deal_py_seed(42))


def oracle_iterations(t, R, S, seed, iter0, n_iters, batch):
    """Tree.mccfr_batched iteration by iteration -> (R, S, the A_row summed over the iterations); the inputs are not modified"""
    R, S, A = np.array(R, np.float64), np.array(S, np.float64), np.zeros((t.n_infosets, 4))
    for it in range(iter0, iter0 + n_iters):
        dR, dS, dA, _, _ = t.mccfr_batched_delta_abs(R, seed, it, 0, batch)
        R += dR
        S += dS
        A += dA
    return R, S, A


def check_iterations(got, t, R0, S0, seed, iter0, n_iters, batch, what, exact_strategy=True):
    """tables `got` = (R, S) after n_iters batched iterations from (R0, S0): test_gpu_mccfr_edges.py's _check_applied for one iteration through
    k_mccfr_apply (strategy sums exact), its _check_iterations for several iterations and (exact_strategy=False) for one iteration of the other
    apply kernels, which that module holds to the several-iteration form"""
    Ro, So, A = oracle_iterations(t, R0, S0, seed, iter0, n_iters, batch)
    Rg, Sg = got
    err = np.abs(Rg - Ro)
    if n_iters == 1 and exact_strategy:
        tol = E.K_REORDER * E.EPS * A.sum(1)[:, None] + 2 * E.EPS * np.abs(Ro)
        count = np.rint((So - S0).sum(1))
        want_S = S0 + count[:, None] * E.reference_sigma(np.asarray(R0, np.float64), t.infoset_nlegal)
        assert np.array_equal(Sg, want_S), (what, "strategy sums")
    else:
        tol = 100 * E.K_REORDER * E.EPS * A.sum(1)[:, None] + 100 * n_iters * E.EPS * np.abs(Ro)
        np.testing.assert_allclose(Sg, So, rtol=1e-10, atol=1e-10, err_msg=str(what))
    print(f"{what}: largest regret error / tolerance {np.max(err / np.maximum(tol, 1e-300)):.3g}")
    assert (err <= tol).all(), (what, np.argwhere(err > tol)[:4])
    return tol


def counted(ctx, before, pairs, what):
    """the context's counters moved by exactly `pairs` traversal pairs since `before`"""
    now = ctx.counters()
    assert (now[0] - before[0], now[1] - before[1]) == (PAIR[0] * pairs, PAIR[1] * pairs), what
    return now
