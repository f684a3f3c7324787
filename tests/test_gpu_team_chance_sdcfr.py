"""Deep CFR on Team MiniScopa over a set of deals on the GPU: scopa_team_chance_sdcfr_traverse (k_team_chance_sdcfr_policy, k_team_chance_sdcfr_walk),
scopa_team_chance_sdcfr_average_policy and TeamChanceDeepCFR, against tests/team_sdcfr_ref.py -- the restatement that tests/test_team_sdcfr_ref.py
holds to the reference's own run.

Tolerances.  The project's ATOL = 1e-5 on an advantage moves pos / z by at most 5 ATOL / z, so policies are compared at rows whose float64
positive-advantage sum z is at least 1e-3 with |dp| <= 5e-5 / z; at most 2 % of the rows may fall below (the CPU test asserts that of the float64
reference for the nets used here) and those must still sum to 1 or 0 and be zero beyond the legal count.  Thresholds are compared bit for bit with
the rule applied to the device's own float32 row.  The walk is compared with the restatement run on the DEVICE's tables under the library's Philox
keying: features, masks, ring positions and visits exactly, regrets and root values to ATOL."""
import ctypes as C

import numpy as np
import pytest

import mccfr_edges as E
import team_chance_sets as TS
import team_sdcfr_ref as S

pytestmark = pytest.mark.gpu

ATOL = 1e-5
ROWS = S.ROWS
SEED, ITERATION = S.TSD_SEED, 3
SENTINEL = -7.5
M32 = 0xFFFFFFFF
NL = S.legal_count_of_rows()
LEGAL = np.arange(4)[None, :] < NL[:, None]


class World:
    """`reordered` (2 deals), `both4` (4 deals) and a one-deal handle holding reordered's deal 1 on one context of its own stream; the fixture's nets
    and the zero-sum nets (head bias -10) as packed images"""

    def __init__(self, sl):
        import torch
        self.sl, self.torch = sl, torch
        self.stream = torch.cuda.Stream(device=0)
        self.ctx = sl.Context(0, stream=self.stream.cuda_stream)
        self.ctx.mccfr_seed(SEED)
        self.perms = {"reordered": TS.deal_set("reordered"), "both4": TS.deal_set("both4")}
        self.perms["one"] = self.perms["reordered"][1:2]
        self._games = {}
        self.nets = {"golden": S.golden_nets(), "zero": [S.with_head_bias(n, -10.0) for n in S.golden_nets()]}
        self.images = {k: self.pack(v) for k, v in self.nets.items()}

    def game(self, name):
        if name not in self._games:
            self._games[name] = self.sl.TeamChanceGame(self.perms[name], self.ctx)
        return self._games[name]

    def device_net(self, net):
        return [self.torch.from_numpy(np.ascontiguousarray(net[k])).cuda().contiguous() for k in ("w1", "b1", "w2", "b2", "w3", "b3")]

    def pack(self, nets):
        torch = self.torch
        image = torch.zeros((2, self.sl.lib().scopa_sdcfr_image_floats()), dtype=torch.float32, device="cuda:0")
        keep = [self.device_net(n) for n in nets]
        torch.cuda.synchronize()
        for p, t in enumerate(keep):
            self.ctx.sdcfr_pack_weights(p, *(x.data_ptr() for x in t), image.data_ptr())
        self.ctx.synchronize()
        return image

    def rings(self, capacity):
        torch = self.torch
        return [torch.full((capacity, w), SENTINEL, dtype=torch.float32, device="cuda:0") for w in (34, 16, 16)]

    def call(self, name, traverser, batch, deals, capacity, write_base, with_mask, nets="golden", iteration=ITERATION, b0=0):
        """-> (feat, regret, mask or None, root values) as numpy after one traversal call into sentinel-filled rings"""
        torch, g = self.torch, self.game(name)
        m = g.n if deals is None else len(deals)
        f, r, k = self.rings(capacity)
        v = torch.full((m * batch,), SENTINEL, dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        g.sdcfr_traverse(traverser, batch, self.images[nets].data_ptr(), f.data_ptr(), r.data_ptr(), k.data_ptr() if with_mask else 0, capacity, write_base,
                         v.data_ptr(), iteration, b0, deals)
        self.ctx.synchronize()
        return f.cpu().numpy(), r.cpu().numpy(), k.cpu().numpy() if with_mask else None, v.cpu().numpy()

    def close(self):
        for g in self._games.values():
            g.close()
        self.ctx.close()


@pytest.fixture(scope="module")
def world(sl):
    try:
        w = World(sl)
    except sl.ScopaError as e:
        if e.status == sl.SCOPA_ENODEV:
            pytest.skip("no GPU on this box")
        raise
    yield w
    w.close()


def feature_bits(f):
    """[N][34] float32 rows -> uint32 bits, after checking that they are 0 / 1 with [32] = 1 and [33] = 0"""
    assert np.isin(f, (0.0, 1.0)).all() and (f[:, 32] == 1.0).all() and (f[:, 33] == 0.0).all()
    return (f[:, :32].astype(np.uint64) << np.arange(32, dtype=np.uint64)[None, :]).sum(1).astype(np.uint32)


def float64_choice(perms, d):
    return TS.cached(("tsd64", "reordered", d), lambda: S.float64_tables(perms[d], S.golden_nets(), None))


def check_rows_are_policies(pol):
    s = pol.astype(np.float64).sum(1)
    assert (pol[~LEGAL] == 0).all() and (pol >= 0).all()
    assert ((np.abs(s - 1.0) <= 1e-5) | (s == 0)).all()


# ---- 1. the policy table ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("traverser", [0, 1])
def test_policy_table_against_the_float64_forward(world, traverser):
    g, perms = world.game("reordered"), world.perms["reordered"]
    world.call("reordered", traverser, 1, None, 2 * ROWS, 0, False)
    for slot in range(2):
        pol, thr = g.sdcfr_policy_get(slot)
        ref, z, _, _ = float64_choice(perms, slot)
        good = z >= 1e-3
        assert (~good).mean() <= 0.02
        err = np.abs(pol.astype(np.float64) - ref).max(1)
        print(f"traverser {traverser} slot {slot}: max |dp| z at the compared rows {float((err * z)[good].max()):.3e} (bound 5e-5)")
        assert (err[good] <= 5 * ATOL / z[good]).all()
        check_rows_are_policies(pol)
        assert np.array_equal(thr, S.thresholds(pol, NL))
        forced = g.sdcfr_forced_get(slot)
        fref, fz = S.forced64(perms[slot], world.nets["golden"], traverser, stride=8)
        fgood = fz >= 1e-3
        assert (~fgood).mean() <= 0.02 and (np.abs(forced[:, ::8] - fref)[fgood] <= 5 * ATOL / fz[fgood]).all()
        assert ((forced >= 0) & (forced <= 1)).all()


def test_policy_table_of_the_zero_sum_nets(world):
    g = world.game("reordered")
    world.call("reordered", 1, 1, [1, 0], 2 * ROWS, 0, False, nets="zero")
    for slot in range(2):
        pol, thr = g.sdcfr_policy_get(slot)
        assert (pol == 0).all() and (thr[:, 0] == S.ZERO_SUM).all() and (thr[:, 1:] == S.TWO53).all()
        assert (g.sdcfr_forced_get(slot) == 0).all()


# ---- 2. the walk ------------------------------------------------------------------------------------------------------------------------------------
def expected_rows(world, name, traverser, batch, deals, iteration, b0, seed):
    """the restatement in mode (b) on the device's own tables of the call just made -> (bits, regrets, values, visits) in slot-major traversal order"""
    g, perms = world.game(name), world.perms[name]
    deals = list(range(g.n)) if deals is None else deals
    bits, regs, vals, visits = [], [], [], 0
    for s, d in enumerate(deals):
        pol, thr = g.sdcfr_policy_get(s)
        forced = g.sdcfr_forced_get(s)
        for i in range(batch):
            tr = S.Traversal(perms[d], traverser, S.table_policy(pol, forced, traverser),
                             S.philox_chooser(thr, traverser, (b0 + d * batch + i) & M32, iteration, seed))
            b, r, _ = tr.arrays()
            assert b.shape[0] == ROWS
            bits.append(b); regs.append(r); vals.append(tr.value)
            visits += int(tr.visits.sum())
    return np.concatenate(bits), np.concatenate(regs), np.array(vals, np.float32), visits


def check_walk(world, name, traverser, batch, deals, with_mask, nets="golden", iteration=ITERATION, b0=0, seed=SEED, write_base=11):
    g = world.game(name)
    m = g.n if deals is None else len(deals)
    n_rows = ROWS * m * batch
    capacity = n_rows + 29
    v0 = g.sdcfr_visits()
    f, r, k, v = world.call(name, traverser, batch, deals, capacity, write_base, with_mask, nets, iteration, b0)
    bits, regs, vals, visits = expected_rows(world, name, traverser, batch, deals, iteration, b0, seed)
    at = (write_base + np.arange(n_rows)) % capacity
    assert np.array_equal(feature_bits(f[at]), bits)
    if with_mask:
        assert np.array_equal(k[at], f[at][:, :16])
    print(f"{name} traverser {traverser} batch {batch}: max |d regret| {float(np.abs(r[at] - regs).max()):.3e}, max |d value| {float(np.abs(v - vals).max()):.3e}")
    np.testing.assert_allclose(r[at], regs, atol=ATOL, rtol=0)
    np.testing.assert_allclose(v, vals, atol=ATOL, rtol=0)
    untouched = np.ones(capacity, bool)
    untouched[at] = False
    assert (f[untouched] == SENTINEL).all() and (r[untouched] == SENTINEL).all() and (k is None or (k[untouched] == SENTINEL).all())
    assert g.sdcfr_visits() - v0 == visits == m * batch * S.VISITS[traverser]
    return f, r, k, v


WALKS = {"batch1": ("reordered", 0, 1, None, True), "batch2": ("reordered", 1, 2, None, False), "batch3_one_of_two": ("reordered", 0, 3, [1], True),
         "three_of_four_unordered": ("both4", 1, 2, [3, 0, 2], False)}


@pytest.mark.parametrize("case", list(WALKS))
def test_walk_rows_against_the_restatement(world, case):
    check_walk(world, *WALKS[case])


@pytest.mark.parametrize("traverser", [0, 1])
def test_walk_with_workgroups_that_take_several_traversals(world, traverser):
    """two workgroups per slot for five traversals: a workgroup walks three or two of them in turn"""
    g = world.game("reordered")
    g.debug_sdcfr(walk_groups=2)
    try:
        check_walk(world, "reordered", traverser, 5, None, traverser == 0)
    finally:
        g.debug_sdcfr()


@pytest.mark.parametrize("traverser", [0, 1])
def test_walk_under_the_zero_sum_nets(world, traverser):
    """every opponent visit takes numpy's uniform arithmetic; every node of the traverser has value 0"""
    f, r, k, v = check_walk(world, "reordered", traverser, 2, None, False, nets="zero")
    assert (v == 0).all()


@pytest.mark.parametrize("seed,iteration,b0", S.word_cases(2, 2), ids=lambda w: hex(w))
def test_walk_under_wide_philox_words(world, seed, iteration, b0):
    """one wide word at a time, then all: tests/test_team_sdcfr_ref.py asserts that these rows are not the ones a narrowed word gives"""
    world.ctx.mccfr_seed(seed)
    try:
        check_walk(world, "reordered", 1, 2, None, False, iteration=iteration, b0=b0, seed=seed)
    finally:
        world.ctx.mccfr_seed(SEED)


# ---- 3. invariance ------------------------------------------------------------------------------------------------------------------------------------
def _same(a, b):
    return all((x is None and y is None) or np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("traverser", [0, 1])
def test_a_deals_traversals_do_not_depend_on_the_list(world, traverser):
    batch, b0 = 3, 40
    n = ROWS * batch
    out = {}
    for name, deals in {"all": None, "swapped": [1, 0], "alone": [1]}.items():
        s = {"all": 1, "swapped": 0, "alone": 0}[name]
        f, r, k, v = world.call("reordered", traverser, batch, deals, 2 * n, 0, True, b0=b0)
        out[name] = (f[s * n:(s + 1) * n], r[s * n:(s + 1) * n], k[s * n:(s + 1) * n], v[s * batch:(s + 1) * batch])
    assert _same(out["all"], out["swapped"]) and _same(out["all"], out["alone"])
    # the one-deal handle holding that deal: its deal 0 has the ids b0' + i, so b0' = b0 + 1 * batch; rows at write_base shifted by the slot
    f, r, k, v = world.call("one", traverser, batch, None, 2 * n, n, True, b0=b0 + batch)
    assert _same(out["all"], (f[n:], r[n:], k[n:], v)) and (f[:n] == SENTINEL).all()
    # no mask stream: the same features and regrets; two runs: the same bits
    again = world.call("reordered", traverser, batch, [1], 2 * n, 0, False, b0=b0)
    assert again[2] is None and _same(out["alone"][:2], (again[0][:n], again[1][:n])) and np.array_equal(again[3], out["alone"][3])
    assert np.array_equal(out["all"][2], out["all"][0][:, :16])
    other = world.call("reordered", traverser, batch, [0], 2 * n, 0, True, b0=b0)
    assert not np.array_equal(other[1][:n], out["alone"][1])                # another deal does not give these rows


# ---- 4. the ring --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("traverser", [0, 1])
def test_ring_wrap_inside_a_traversal(world, traverser):
    batch = 2
    rows = ROWS * 2 * batch
    capacity = rows + 7
    write_base = capacity - (ROWS + 700)                                    # the ring wraps 700 rows into the second traversal of slot 0
    flat = world.call("reordered", traverser, batch, None, rows, 0, True)
    f, r, k, v = world.call("reordered", traverser, batch, None, capacity, write_base, True)
    at = (write_base + np.arange(rows)) % capacity
    assert at[ROWS + 699] == capacity - 1 and at[ROWS + 700] == 0
    assert np.array_equal(f[at], flat[0]) and np.array_equal(r[at], flat[1]) and np.array_equal(k[at], flat[2]) and np.array_equal(v, flat[3])
    untouched = (r == SENTINEL).all(1)
    assert untouched.sum() == 7 and untouched[(write_base + rows) % capacity:write_base].all()
    assert (f[untouched] == SENTINEL).all() and (k[untouched] == SENTINEL).all()


# ---- 5. refusals --------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_ring_alone(world):
    sl, torch = world.sl, world.torch
    L, batch, g = sl.lib(), 2, world.game("both4")
    capacity = ROWS * 4 * batch
    f, r, k = world.rings(capacity)
    v = torch.full((4 * batch,), SENTINEL, dtype=torch.float32, device="cuda:0")
    image = world.images["golden"]
    torch.cuda.synchronize()
    P = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None

    def call(deals, m=None, traverser=0, batch=batch, capacity=capacity, write_base=0, b0=0, image_ptr=P(image), feat=P(f), regret=P(r), mask=P(k), root=P(v)):
        d = None if deals is None else np.ascontiguousarray(deals, np.int32)
        m = (0 if d is None else d.size) if m is None else m
        L.scopa_last_error(world.ctx._h)
        rc = L.scopa_team_chance_sdcfr_traverse(g._h, traverser, batch, m, None if d is None else d.ctypes.data_as(C.c_void_p), image_ptr, feat, regret, mask,
                                                capacity, write_base, root, ITERATION, b0)
        return rc, L.scopa_last_error(world.ctx._h).decode()

    off = lambda t, b: C.c_void_p(t.data_ptr() + b)
    cases = {"traverser 2": call(None, traverser=2), "traverser -1": call(None, traverser=-1), "a negative batch": call(None, batch=-1),
             "batch 0 with a list": call([1], batch=0), "a list with m = 0": call([0], m=0), "m above n": call([0, 1, 2, 3, 0], m=5),
             "no list with m = 2": call(None, m=2), "a duplicate id": call([1, 3, 1]), "an id equal to n": call([0, 4]), "a negative id": call([-1]),
             "no image": call(None, image_ptr=None), "no feature ring": call(None, feat=None), "no regret ring": call(None, regret=None),
             "no root values": call(None, root=None), "a misaligned image": call(None, image_ptr=off(image, 4)),
             "a misaligned d_mem_feat": call(None, feat=off(f, 4)), "a misaligned d_mem_regret": call(None, regret=off(r, 8)),
             "a misaligned d_mem_mask": call(None, mask=off(k, 4)), "a ring below one traversal": call([0], batch=1, capacity=ROWS - 1),
             "a ring of 2^30 rows": call([0], batch=1, capacity=1 << 30), "write_base = capacity": call(None, write_base=capacity),
             "a negative write_base": call(None, write_base=-1), "a ring too small": call(None, capacity=capacity - 1),
             "b0 overflow": call(None, b0=2 ** 32 - 4 * batch + 1)}
    for what, (rc, msg) in cases.items():
        assert rc == sl.SCOPA_EINVAL and msg.startswith("scopa_team_chance_sdcfr_traverse:"), (what, rc, msg)
    world.ctx.synchronize()
    for t in (f, r, k, v):
        assert bool((t == SENTINEL).all())
    assert call(None, batch=0)[0] == sl.SCOPA_OK                                                    # batch 0 without a list: a no-op
    world.ctx.synchronize()
    assert bool((r == SENTINEL).all())
    assert call(None, b0=S.last_b0(4, batch))[0] == sl.SCOPA_OK                                     # the last id is 2^32 - 1: accepted
    world.ctx.synchronize()
    assert bool((r != SENTINEL).all()) and bool((v != SENTINEL).all())


def test_policy_get_refusals(world):
    sl = world.sl
    g = sl.TeamChanceGame(world.perms["one"], world.ctx)
    try:
        with pytest.raises(sl.ScopaError) as e:
            g.sdcfr_policy_get(0)
        assert e.value.status == sl.SCOPA_ESTATE
        with pytest.raises(sl.ScopaError) as e:
            g.sdcfr_forced_get(0)
        assert e.value.status == sl.SCOPA_ESTATE
    finally:
        g.close()
    world.call("reordered", 0, 1, [1], ROWS, 0, False)
    for slot in (-1, 1):
        with pytest.raises(sl.ScopaError) as e:
            world.game("reordered").sdcfr_policy_get(slot)
        assert e.value.status == sl.SCOPA_EINVAL


# ---- 6. the average policy over keys ------------------------------------------------------------------------------------------------------------------
STORE = [S.random_net(100 + s, head_bias=0.3) for s in range(5)]
AVERAGES = {"none": ([], []), "one": ([3], [1.0]), "three": ([4, 0, 2], [0.5, 0.3, 0.2]), "slot_outside_the_store": ([4, 7, 2], [0.5, 0.3, 0.2])}


def average_table(world, slots, coef, teams=(0, 1)):
    torch, g = world.torch, world.game("reordered")
    n = len(slots)
    store = [torch.stack([world.device_net(net)[i] for net in STORE]).contiguous() for i in range(6)]
    d_slots = torch.tensor(slots if n else [0], dtype=torch.int32, device="cuda:0")
    d_coef = torch.tensor(coef if n else [0.0], dtype=torch.float32, device="cuda:0")
    out = torch.full((g.G, 4), float("nan"), dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    for t in teams:
        g.sdcfr_average_policy(t, n, [x.data_ptr() for x in store] if n else [0] * 6, len(STORE), d_slots.data_ptr() if n else 0, d_coef.data_ptr() if n else 0,
                               out.data_ptr())
    world.ctx.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("case", list(AVERAGES))
def test_average_policy_over_keys(world, case):
    """against the float64 restatement at the well-conditioned keys.  A term's policy moves by at most 5 ATOL / z_s, the FIFO sum acc_k by
    E = sum coef_s 5 ATOL / z_s, the legal slots' total T by at most 4 E, so acc_k / T by at most (E + 4 E) / T = 5 E / T; float32 rounding of the
    products and sums adds a few 1e-7"""
    g, cr, perms = world.game("reordered"), TS.chance_ref("reordered"), world.perms["reordered"]
    slots, coef = AVERAGES[case]
    keys, mp = g.index()
    assert np.array_equal(keys, cr.gkey) and np.array_equal(mp, cr.map)
    one = average_table(world, slots, coef, teams=(1,))
    assert np.isnan(one[cr.team == 0]).all() and not np.isnan(one[cr.team == 1]).any()          # the other team's rows are left alone
    G = average_table(world, slots, coef)
    assert np.array_equal(G[cr.team == 1], one[cr.team == 1]) and not np.isnan(G).any()
    legal = np.arange(4)[None, :] < cr.nleg[:, None]
    assert (G[~legal] == 0).all() and np.abs(G.sum(1) - 1.0).max() <= 1e-15
    uniform = np.where(legal, 1.0 / cr.nleg[:, None], 0.0)
    if case in ("none", "slot_outside_the_store"):
        assert np.array_equal(G, uniform)
    else:
        for team in (0, 1):
            rows, ref, z = S.average_policy(cr, perms, team, [STORE[s] for s in slots], coef)
            good = (z >= 1e-3).all(0)
            assert (~good).mean() <= 0.02
            E = (np.array(coef)[:, None] * 5 * ATOL / np.maximum(z, 1e-3)).sum(0)
            err = np.abs(G[rows] - ref).max(1)
            print(f"{case} team {team}: max |dp| {float(err[good].max()):.3e}")
            assert (err[good] <= 5 * E[good] / sum(coef) + 1e-6).all()
        assert not np.array_equal(G, uniform)
        assert np.array_equal(average_table(world, slots, coef), G)                             # no atomics: the same bits from run to run
        g.debug_sdcfr(terms_bytes=16 * len(slots) * 4096)                                       # chunks of 4 096 keys: the same bits
        try:
            assert np.array_equal(average_table(world, slots, coef), G)
        finally:
            g.debug_sdcfr()
    out = g.exploitability(G)
    assert np.isfinite(out).all() and out[0] >= -1e-12
    if case == "none":
        assert np.array_equal(out, g.exploitability(uniform))


# ---- 7. TeamChanceDeepCFR -----------------------------------------------------------------------------------------------------------------------------
def test_team_chance_deep_cfr(world):
    import inspect
    import torch
    from scopa_amd.algorithms.deep_cfr import TeamChanceDeepCFR
    from scopa_amd.algorithms.deep_cfr.chance_deep_cfr import iteration_deals
    from scopa_amd.algorithms.deep_cfr.team_chance_deep_cfr import default_memory_size
    sl = world.sl

    cm = TS.chance_mc_ref("reordered")
    bits = lambda a: np.ascontiguousarray(a, np.float64).view(np.uint64)

    def tabular(game, what):
        """two CFR iterations from reset -> their tables, bit-reproducible; then one MCCFR iteration held to the restatement from the device's own
        tables as tests/test_gpu_team_chance_mccfr.py holds it: strategy sums bit for bit, regrets (float64 atomics, added in arrival order) within the
        project's reorder budget K_REORDER * eps * A_row + 2 eps |R|"""
        game.tables_reset()
        game.cfr_iterate(2)
        R0, S0 = game.tables_get()
        R, S, sig, it = R0.copy(), S0.copy(), game.sigma_get(), game.mccfr_counters()[2]
        A, cnt = cm.iterate(R, S, sig, 2, SEED, it, None)
        game.mccfr_iterate(2, 1)
        Rg, Sg = game.tables_get()
        assert np.array_equal(bits(Sg), bits(S)) and game.mccfr_counters()[2] == it + 1, what
        bound = (E.K_REORDER * E.EPS * A.sum(1))[:, None] + 2.0 * E.EPS * np.abs(R)
        assert (np.abs(Rg - R) <= bound).all() and cnt.sum() > 0, what
        return R0, S0

    fresh = sl.TeamChanceGame(world.perms["reordered"], world.ctx)
    used = sl.TeamChanceGame(world.perms["reordered"], world.ctx)
    try:
        world.ctx.mccfr_seed(SEED)
        before = tabular(used, "before")
        torch.manual_seed(3)
        d = TeamChanceDeepCFR(used, batch=2, seed=SEED)
        assert d.batch == 2 and inspect.signature(TeamChanceDeepCFR.__init__).parameters["batch"].default == 64
        assert d.advantage_nets[0].buffer.capacity == default_memory_size(2, 2) == 100000 and default_memory_size(24, 64) == 8 * 1653 * 24 * 64
        d.train(iterations=3, advantage_epochs=2)
        h = d.training_history
        assert all(len(h[k][p]) == 3 for k in ("losses", "values", "buffer_sizes") for p in range(2))
        assert h["buffer_sizes"][0] == [ROWS * 2 * 2 * (i + 1) for i in range(3)] == h["buffer_sizes"][1]
        assert d.deal_log == [(0, None), (1, None), (2, None)]
        assert d.strategy_buffers[0].weights == [2, 3] == d.strategy_buffers[1].weights       # none at the call's first iteration, weight = loop index + 1
        assert used.sdcfr_visits() == 3 * 2 * 2 * sum(S.VISITS)
        G = d.policy_table()
        keys, _ = used.index()
        nl = 4 - ((keys >> np.uint64(60)).astype(np.int64) >> 2)
        legal = np.arange(4)[None, :] < nl[:, None]
        assert G.shape == (used.G, 4) and (G[~legal] == 0).all() and np.abs(G.sum(1) - 1.0).max() <= 1e-12
        e = d.exploitability()
        out = used.exploitability(G)
        assert np.isfinite(out).all() and e == dict(exploitability=float(out[0]), br0=float(out[1]), br1=float(out[2]), value_p0=float(out[3]))
        print("TeamChanceDeepCFR on `reordered` after 3 iterations:", e)
        assert np.array_equal(d.policy_table_for(fresh), G)                                    # the same keys on another handle: the same table
        reward, scopas = d.evaluate_vs_random(64)
        assert np.isfinite(reward) and len(scopas) == 2 and abs(d.last_eval_exact_reward) <= 20
        d.train(iterations=1, advantage_epochs=1, exploitability_freq=1)
        assert [i for i, _ in h["exploitability"]] == [3] and np.isfinite(h["exploitability"][0][1])
        # a deal per iteration: the lists are iteration_deals'
        torch.manual_seed(3)
        s = TeamChanceDeepCFR(used, batch=2, deals_per_iteration=1, seed=SEED)
        s.train(iterations=3, advantage_epochs=1)
        assert [i for i, _ in s.deal_log] == [0, 1, 2]
        assert all(np.array_equal(x, iteration_deals(2, 1, i, SEED)) and len(x) == 1 for i, x in s.deal_log)
        assert s.training_history["buffer_sizes"][1] == [ROWS * 2 * (i + 1) for i in range(3)]
        # the tabular solvers on the same handle give a fresh handle's bits, before and after
        world.ctx.mccfr_seed(SEED)
        after = tabular(used, "after")
        first, second = tabular(fresh, "fresh, first"), tabular(fresh, "fresh, second")
        for got, want in ((before, first), (after, second)):
            assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(got, want))
    finally:
        used.close()
        fresh.close()
        world.ctx.mccfr_seed(SEED)
