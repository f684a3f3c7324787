"""GPU checks of the FullScopa solver's infoset STORE (scopa_amd/csrc/scopa_full_store.h: fm_hash, fm_find, fm_claim; scopa_full_store_host.h:
k_full_store_import and k_full_store_export) on probe chains built slot by slot, and of the walk and the match on such stores against the restatement
tests/full_mccfr_ref.py.

tests/test_gpu_full_mccfr.py checks the walk on stores that are nearly empty.  Here the home slot of a key is restated (F.home_slot), filler keys that play
never meets are searched for a wanted home (F.fillers), and the stores are built so that what they hold is SURE, whatever order the lanes arrive in:

  * a probe never looks past the first free slot after its home in the final occupied set, so while that distance (F.Store.reach) is at most 64 for every
    key, every key is held; the CPU guards of tests/test_full_mccfr_ref.py assert it for every store built here;
  * 64 fillers of one home h fill exactly h .. h + 63 when no other key has its home near (F.isolated); a 65th key of that home is dropped for sure.

The probe length of the SEQUENTIAL model (F.Store.probe) is not such a guard, because it depends on the insertion order.  Two of the stores first asked
for (64 keys of home 2^10 - 3 with 10 of home 0; 40 of home h with 40 of home h + 20) cannot be held whole under a limit of 64 slots in every order -- the
first in no order at all: its 74 keys can reach 67 slots.  They are kept with what IS sure about them (test_literal_overfull_chains), next to stores of the
same shape that fit (54 + 10 across the wrap, 40 + 24 touching).  The restatement is itself under test here: a 65th key of one restated home is dropped at
2^10 slots only if the device hashes as F.home_slot does."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest

import full_mccfr_ref as F
import philox_words as W
from test_gpu_full_mccfr import SEED, assert_delta, planted, ref_delta, root_of, rows_from_device, same_bits, solver_of

pytestmark = pytest.mark.gpu

C_SMALL, C_BIG = 10, 18
WRAP_HOME, TOUCH_HOME = (1 << C_SMALL) - 3, 500
MATCH_NS, MATCH_STREAM = (1, 2, 63, 65, 129), (1 << 24) - 1
BLOCKED_LAUNCHES = ((42, 0), (7, 1))                                        # (deck seed, traverser) at round 3, nb 8


# ---- the stores (CPU; tests/test_full_mccfr_ref.py guards each) ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def small_stores():
    """name -> keys of the stores of section 1 at 2^10 slots that are held whole for sure"""
    wrap, zero = F.fillers(WRAP_HOME, 64, C_SMALL, 1), F.fillers(0, 10, C_SMALL, 2)
    a, b = F.fillers(TOUCH_HOME, 40, C_SMALL, 3), F.fillers(TOUCH_HOME + 20, 40, C_SMALL, 4)
    c = np.random.RandomState(1).randint(0, 1 << 40, size=640, dtype=np.int64).astype(np.uint64)
    return dict(chain=F.fillers(512, 64, C_SMALL, 5), wrap64=wrap, wrap=np.concatenate([wrap[:54], zero]), touch=np.concatenate([a, b[:24]]),
                mixed=np.uint64(F.FILLER_BASE) | (c << np.uint64(16)), ten=F.fillers(100, 10, C_SMALL, 6))


@functools.lru_cache(maxsize=None)
def overfull_stores():
    """name -> (keys, slots the keys can reach): the two stores that were asked for and cannot be held whole in every arrival order"""
    wrap, zero = F.fillers(WRAP_HOME, 64, C_SMALL, 1), F.fillers(0, 10, C_SMALL, 2)
    a, b = F.fillers(TOUCH_HOME, 40, C_SMALL, 3), F.fillers(TOUCH_HOME + 20, 40, C_SMALL, 4)
    return dict(wrap=(np.concatenate([wrap, zero]), 67), touch=(np.concatenate([a, b]), 84))


@functools.lru_cache(maxsize=None)
def chained_planted(oracle):
    """the planted tables of test_gpu_full_mccfr.planted (deck 42, round 4) with every key chosen as the first in ascending order that has the row's shape
    AND is isolated at 2^18 among the keys of the launches below; fill = 63 fillers of each key's home; launch[trav] = the restatement at nb 24 under the
    planted rows.  A key is None where no candidate is isolated (the CPU guard asserts there is none such)"""
    root, _, n_act, R, S = planted(oracle)
    seen = F.Rows()
    for trav in range(2):
        F.traverse(root, trav, 0, 0, 4, SEED, seen)
    zero = set()
    for trav in range(2):
        zero |= set(ref_delta(oracle, 42, 4, trav, 0, 0, 24, SEED).count)
    shapes = (lambda k: k == F.key_of(root, 0), lambda k: (k >> 62) & 1 == 1 and F.key_actions(k) == 3,
              lambda k: (k >> 62) & 1 == 0 and F.key_actions(k) == 2, lambda k: (k >> 62) & 1 == 1 and F.key_actions(k) == 2)
    K = [next((k for k in sorted(seen.count) if shape(k) and F.isolated(k, zero, C_BIG)), None) for shape in shapes]
    fx = SimpleNamespace(root=root, K=K, n_act=n_act, R=R, S=S, zero=zero, launch=[], fill=None)
    if None not in K:
        fx.K = np.array(K, np.uint64)
        fx.fill = np.concatenate([F.fillers(F.home_slot(k, C_BIG), 63, C_BIG, 1 + i) for i, k in enumerate(fx.K)])
        for trav in range(2):
            rows = F.Rows()
            rows.plant(fx.K, R, S)
            F.traverse(root, trav, 0, 0, 24, SEED, rows)
            fx.launch.append(rows)
    return fx


@functools.lru_cache(maxsize=None)
def blocked_launch(oracle, deck_seed, trav):
    """round 3, nb 8: base = the restatement on an empty store; blocked = (the first isolated traverser key met more than once, the first isolated key
    of the opponent's first node of the round), first as the walk meets them; fill = 64 fillers at the home of each; rows = the restatement with the
    two keys absent"""
    base = ref_delta(oracle, deck_seed, 3, trav, 0, 0, 8, SEED)
    met = list(base.count)
    k_trav = next((k for k in met if (k >> 62) & 1 == trav and base.count[k] > 1 and F.isolated(k, met, C_BIG)), None)
    k_opp = next((k for k in met if (k >> 62) & 1 != trav and (k >> 59) & 7 == 3 and F.key_actions(k) == 3 and F.isolated(k, met, C_BIG)), None)
    fx = SimpleNamespace(root=root_of(oracle, deck_seed, 3)[2], base=base, blocked=(k_trav, k_opp), fill=None, rows=None)
    if None not in fx.blocked:
        fx.fill = np.concatenate([F.fillers(F.home_slot(k, C_BIG), 64, C_BIG, 1 + i) for i, k in enumerate(fx.blocked)])
        fx.rows = F.Rows()
        F.traverse(fx.root, trav, 0, 0, 8, SEED, fx.rows, absent=frozenset(fx.blocked))
    return fx


# ---- helpers ---------------------------------------------------------------------------------------------------------------------------------------------
def set_rows(h, keys):
    R, S = F.rows_for(keys)
    h.tables_set(keys, [F.key_actions(k) for k in keys], R, S)


def assert_own_rows(got, what):
    """every row that came back carries the values F.rows_for gives its key, the action count of its key, and no key twice"""
    keys, n_act, R, S = got
    want = F.rows_for(keys)
    assert np.unique(keys).size == keys.size and list(n_act) == [F.key_actions(k) for k in keys], what
    assert same_bits(R, want[0]) and same_bits(S, want[1]), f"{what}: a row came back with another key's values"


def assert_holds(h, keys, dropped, what):
    """the store holds exactly `keys`, each with its own row, and the counters say so"""
    got = h.tables_get()
    assert np.array_equal(got[0], np.sort(np.asarray(keys, np.uint64))), f"{what}: key sets differ ({got[0].size} rows against {len(keys)})"
    assert_own_rows(got, what)
    c = h.counters()
    assert (c["rows"], c["dropped"]) == (len(keys), dropped), what


def raises(sl, status, fn, *args):
    with pytest.raises(sl.ScopaError) as e:
        fn(*args)
    assert e.value.status == status, e.value


class Visible:
    """a solver seen without the rows in `hidden` (fillers, planted rows the launch does not meet), each of which must show no visit and no increment"""

    def __init__(self, h, hidden):
        self.h, self.hidden = h, np.asarray(sorted(int(k) for k in hidden), np.uint64)

    def delta_get(self):
        keys, counts, dR, dS = self.h.delta_get()
        hid = np.isin(keys, self.hidden)
        assert hid.sum() == self.hidden.size and not counts[hid].any() and not dR[hid].any() and not dS[hid].any(), "a row no walk meets was changed or is gone"
        return keys[~hid], counts[~hid], dR[~hid], dS[~hid]

    def tables_get(self):
        got = self.h.tables_get()
        return tuple(x[~np.isin(got[0], self.hidden)] for x in got)


# ---- 1. the store alone ------------------------------------------------------------------------------------------------------------------------------------
def test_chain_of_exactly_64_and_one_more(ctx, sl, oracle):
    h, _ = solver_of(ctx, sl, oracle, 42, 4, capacity_log2=C_SMALL)
    chain, d0 = small_stores()["chain"], h.counters()["dropped"]
    set_rows(h, chain)
    assert_holds(h, chain, d0, "64 keys of one home")
    more = F.fillers(512, 65, C_SMALL, 5)
    assert np.array_equal(more[:64], chain) and np.unique(more).size == 65
    raises(sl, sl.SCOPA_ENOMEM, set_rows, h, more)
    got, c = h.tables_get(), h.counters()
    assert (got[0].size, c["rows"], c["dropped"]) == (64, 64, d0 + 1) and np.isin(got[0], more).all()
    assert_own_rows(got, "65 keys of one home")
    ten = small_stores()["ten"]
    set_rows(h, ten)                                                       # no error: the drop before was reported once
    assert_holds(h, ten, d0 + 1, "10 keys after a drop")


@pytest.mark.parametrize("name", ["wrap64", "wrap", "touch"])
def test_chains_across_the_wrap_and_touching(ctx, sl, oracle, name):
    """wrap64: 64 keys of home 2^10 - 3 (slots 1021 .. 1023, 0 .. 60).  wrap: 54 of that home and 10 of home 0, the same 64 slots, each group walking past the
    other's keys.  touch: 40 of home h and 24 of home h + 20"""
    h, _ = solver_of(ctx, sl, oracle, 42, 4, capacity_log2=C_SMALL)
    keys, d0 = small_stores()[name], h.counters()["dropped"]
    set_rows(h, keys)
    assert_holds(h, keys, d0, name)
    if name == "wrap":                                                     # apply on a chained store: an ordinary launch over every slot
        h.apply()
        assert_holds(h, keys, d0, "after apply")
        _, counts, dR, dS = h.delta_get()
        assert counts.size == keys.size and not counts.any() and not dR.any() and not dS.any()


@pytest.mark.parametrize("name", ["wrap", "touch"])
def test_literal_overfull_chains(ctx, sl, oracle, name):
    """64 keys of home 2^10 - 3 with 10 of home 0 (74 keys that can reach 67 slots), and 40 of home h with 40 of home h + 20 (held whole only if the first
    group arrives first).  Which keys are dropped depends on the arrival order.  Sure in every order: a key is dropped only after 64 occupied slots, so a call
    that drops leaves at least 64 rows; the rows lie in the slots the keys can reach; every key is either held, with its own row, or counted as dropped"""
    keys, reachable = overfull_stores()[name]
    h, _ = solver_of(ctx, sl, oracle, 42, 4, capacity_log2=C_SMALL)
    d0 = h.counters()["dropped"]
    try:
        set_rows(h, keys)
        status = sl.SCOPA_OK
    except sl.ScopaError as e:
        status = e.status
    got, c = h.tables_get(), h.counters()
    dropped = c["dropped"] - d0
    print(name, "rows", c["rows"], "dropped", dropped)
    assert status == (sl.SCOPA_ENOMEM if dropped else sl.SCOPA_OK) and (name != "wrap" or dropped >= keys.size - reachable)
    assert c["rows"] == got[0].size == keys.size - dropped and 64 <= c["rows"] <= reachable and np.isin(got[0], keys).all()
    assert_own_rows(got, name)


def test_mixed_load_reset_and_three_rows(ctx, sl, oracle):
    h, _ = solver_of(ctx, sl, oracle, 42, 4, capacity_log2=C_SMALL)
    keys, d0 = small_stores()["mixed"], h.counters()["dropped"]
    set_rows(h, keys)
    assert_holds(h, keys, d0, "640 keys in 1024 slots")
    h.reset()
    assert_holds(h, keys[:0], d0, "after reset")
    set_rows(h, keys[100:103])
    assert_holds(h, keys[100:103], d0, "3 keys after reset")


def test_smallest_store(ctx, sl, oracle):
    """2^4 slots: a probe of 64 laps the table, so 16 keys of any homes fit; n_rows above the capacity is refused before the store is touched"""
    keys = small_stores()["mixed"][:17]
    h, _ = solver_of(ctx, sl, oracle, 42, 4, capacity_log2=4)
    set_rows(h, keys[:16])
    assert_holds(h, keys[:16], 0, "16 keys in 16 slots")
    raises(sl, sl.SCOPA_EINVAL, set_rows, h, keys)
    assert_holds(h, keys[:16], 0, "after a refused call")
    rows = ref_delta(oracle, 42, 4, 0, 0, 0, 1, SEED)
    assert len(rows.count) > 16
    h2, _ = solver_of(ctx, sl, oracle, 42, 4, capacity_log2=4)
    raises(sl, sl.SCOPA_ENOMEM, h2.traverse, 0, 0, 0, 1)
    c = h2.counters()
    got, counts, _, _ = h2.delta_get()
    assert c["rows"] == got.size == 16 and all(k in rows.count for k in got.tolist())
    assert int(counts.sum()) + c["dropped"] == c["choice_visits"] == F.shape_counts(4)[0] == rows.choice


def test_tables_set_refusals_leave_the_store(ctx, sl, oracle):
    """every refusal of tables_set, on 3 planted rows in the smallest store (2^4 slots): a key twice, a key without the marker bit, an action count that
    is not the key's, n_rows above the capacity, each array NULL with n_rows > 0.  Each is SCOPA_EINVAL with its own message, found by the host before
    any device work: after it the store answers counters() and holds what it held"""
    _, K, n_act, R, S = planted(oracle)
    K, n_act, R, S = K[:3], n_act[:3], R[:3], S[:3]
    h, _ = solver_of(ctx, sl, oracle, 42, 4, capacity_log2=4)
    h.tables_set(K, n_act, R, S)
    h.apply()
    before = (h.tables_get(), h.delta_get(), h.counters())
    assert (before[2]["rows"], before[2]["iterations"]) == (3, 1)

    def unchanged():
        now = h.tables_get() + h.delta_get()
        return all(x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(now, before[0] + before[1])) and h.counters() == before[2]

    seventeen = small_stores()["mixed"][:17]
    R17, S17 = F.rows_for(seventeen)
    who = "scopa_full_mccfr_tables_set: "
    for bad, message in (((K[[0, 1, 0]], n_act[[0, 1, 0]], R, S), "a key twice"),
                         ((K & np.uint64((1 << 63) - 1), n_act, R, S), "a key without the marker bit, or an action count that is not the key's (2 or 3)"),
                         ((K, [3, 3, 3], R, S), "a key without the marker bit, or an action count that is not the key's (2 or 3)"),
                         ((seventeen, [F.key_actions(k) for k in seventeen], R17, S17), "n_rows outside [0, capacity] or a NULL array")):
        with pytest.raises(sl.ScopaError) as e:
            h.tables_set(*bad)
        assert e.value.status == sl.SCOPA_EINVAL and who + message in str(e.value), e.value
        assert unchanged(), message
    arrays = [K, n_act, R, S]
    for gone in range(4):
        args = [None if i == gone else sl._ptr(a) for i, a in enumerate(arrays)]
        assert sl.lib().scopa_full_mccfr_tables_set(h._h, 3, *args) == sl.SCOPA_EINVAL
        assert sl.lib().scopa_last_error(ctx._h).decode() == who + "n_rows outside [0, capacity] or a NULL array"
        assert unchanged(), gone
    h.tables_set(K, n_act, R, S)                                           # ... and the handle goes on
    assert h.counters()["rows"] == 3


# ---- 2. walks and the match on built stores ----------------------------------------------------------------------------------------------------------------
def test_planted_rows_deep_in_chains(ctx, sl, oracle):
    """each planted row among 63 fillers of its own home: fm_claim (the walk) and fm_find (the prefix replay of cut > 0, the match) must both walk the
    chain to it.  One that gave up early would read a zero row: uniform play at the root, where the planted row plays slot 1 only"""
    fx = chained_planted(oracle)
    keys = np.concatenate([fx.K, fx.fill])
    R, S = F.rows_for(fx.fill)
    R, S = np.concatenate([fx.R, R]), np.concatenate([fx.S, S])
    n_act = [F.key_actions(k) for k in keys]
    order = np.argsort(keys)
    h, _ = solver_of(ctx, sl, oracle, 42, 4, capacity_log2=C_BIG)
    d0, nb = h.counters()["dropped"], 24
    for trav in range(2):
        rows = fx.launch[trav]
        unmet = [int(k) for k in fx.K if int(k) not in rows.count]
        for cut in (-1, 0, 1, 2):
            what = f"planted rows in chains, traverser {trav}, cut {cut}"
            h.reset()
            h.tables_set(keys, n_act, R, S)
            h.cut(cut)
            h.traverse(trav, 0, 0, nb)
            assert_delta(Visible(h, fx.fill.tolist() + unmet), rows, what)
            if trav == 1:                                                  # the root row has ONE positive regret: the opponent plays its slot 1 every time
                got = h.delta_get()
                assert rows.dS[int(fx.K[0])] == [0.0, float(nb), 0.0] == got[3][got[0] == fx.K[0]][0].tolist(), what
            c = h.counters()
            assert (c["dropped"], c["rows"]) == (d0, 256 + len(set(rows.count) - set(fx.K.tolist()))), what
            tab = h.tables_get()
            held = np.isin(tab[0], keys)                                   # the rows that were set come back as set: traverse writes increments only
            assert np.array_equal(tab[0][held], keys[order]) and same_bits(tab[2][held], R[order]) and same_bits(tab[3][held], S[order]), what
            assert not tab[2][~held].any() and not tab[3][~held].any()
    # the match on the same store: every planted strategy row is found behind its fillers, and no filler row is ever played
    ctx.mccfr_seed(W.WIDE_SEED)
    table = {int(k): [float(x) for x in s] for k, s in zip(fx.K, fx.S)}
    for n in MATCH_NS:
        sums, r2 = h.match(n, MATCH_STREAM, per_episode=True)
        want_sums, want_r2 = F.match(fx.root, table, n, W.WIDE_SEED, MATCH_STREAM)
        assert np.array_equal(r2, want_r2) and np.array_equal(sums, want_sums), f"match of {n} episodes"
    raises(sl, sl.SCOPA_EINVAL, h.match, 129, 1 << 24)


def test_row_claimed_at_the_last_slot_of_its_probe(ctx, sl, oracle):
    """Where a row lands in a chain set in ONE call depends on the arrival order (the planted rows above mostly win their home slot), so here the order is
    forced: 63 fillers of the root key's home are set first, and the walk then claims the root key in the 64th and last slot a probe looks at.  The first
    launch and apply leave a regret row there, a later one a strategy row.  From then on every launch is restated from the device's own tables: at
    cut > 0 the prefix lanes must find that row with fm_find where lane 0 finds it with fm_claim, and the match must find it too.  A probe loop one slot
    short reads a zero row and plays uniformly at the root"""
    root = root_of(oracle, 42, 4)[2]
    k_root = F.key_of(root, 0)
    fill = F.fillers(F.home_slot(np.uint64(k_root), C_BIG), 63, C_BIG, 9)
    h, _ = solver_of(ctx, sl, oracle, 42, 4, capacity_log2=C_BIG)
    d0, nb = h.counters()["dropped"], 24
    set_rows(h, fill)
    for counter, (trav, cut) in enumerate([(0, 0), (1, 0), (1, 1), (1, 2), (1, -1), (0, 1), (0, 2)]):
        what = f"root row in the 64th slot, launch {counter}, traverser {trav}, cut {cut}"
        rows = rows_from_device(h)
        if counter:
            assert F.sigma_of(rows.R[k_root], 3) != [1.0 / 3] * 3         # the row matters: a probe that misses it plays another sigma
        F.traverse(root, trav, counter, 0, nb, SEED, rows)
        h.cut(cut)
        h.traverse(trav, counter, 0, nb)
        held = h.tables_get()[0]
        assert_delta(Visible(h, [k for k in held.tolist() if k not in rows.count]), rows, what)
        c = h.counters()
        assert (c["dropped"], c["rows"]) == (d0, held.size) and np.isin(fill, held).all(), what
        h.apply()
    real = held[~np.isin(held, fill)]
    assert k_root in real.tolist() and F.isolated(k_root, real, C_BIG) and F.Store(C_BIG).insert(fill).insert([k_root]).probe[k_root] == 64
    assert_own_rows(tuple(x[np.isin(held, fill)] for x in h.tables_get()), "fillers after seven launches")
    ctx.mccfr_seed(W.WIDE_SEED)
    table = {k: s for k, s in rows_from_device(h).S.items() if k in real.tolist()}
    assert sum(table[k_root]) > 1e-12 and max(table[k_root]) != min(table[k_root])
    sums, r2 = h.match(129, MATCH_STREAM, per_episode=True)
    want_sums, want_r2 = F.match(root, table, 129, W.WIDE_SEED, MATCH_STREAM)
    assert np.array_equal(r2, want_r2) and np.array_equal(sums, want_sums)
    assert not np.array_equal(want_r2, F.match(root, {k: s for k, s in table.items() if k != k_root}, 129, W.WIDE_SEED, MATCH_STREAM)[1])


def test_match_on_a_full_64_slot_store(ctx, sl, oracle):
    """2^6 slots, all held by the root key and 63 fillers of its home: every probe of the match wraps (the home is not slot 0), finds the root's row wherever
    it landed, and gives up on every other key after 64 occupied slots, with no empty slot anywhere to stop it"""
    root = root_of(oracle, 42, 4)[2]
    k_root = F.key_of(root, 0)
    home = F.home_slot(np.uint64(k_root), 6)
    keys = np.concatenate([F.fillers(home, 63, 6, 1), np.array([k_root], np.uint64)])
    R, S = F.rows_for(keys)
    S[63] = [0.25, 0.5, 2.0]
    h, _ = solver_of(ctx, sl, oracle, 42, 4, capacity_log2=6, seed=W.WIDE_SEED)
    h.tables_set(keys, [3] * 64, R, S)
    got = h.tables_get()
    order = np.argsort(keys)
    assert home != 0 and np.array_equal(got[0], keys[order]) and same_bits(got[2], R[order]) and same_bits(got[3], S[order]) and h.counters()["rows"] == 64
    sums, r2 = h.match(129, MATCH_STREAM, per_episode=True)
    want_sums, want_r2 = F.match(root, {k_root: [0.25, 0.5, 2.0]}, 129, W.WIDE_SEED, MATCH_STREAM)
    assert np.array_equal(r2, want_r2) and np.array_equal(sums, want_sums)
    assert not np.array_equal(want_r2, F.match(root, {}, 129, W.WIDE_SEED, MATCH_STREAM)[1])
    assert h.counters()["rows"] == 64 and h.counters()["dropped"] == 0     # the match never inserts, and never counts a drop


@pytest.mark.parametrize("deck_seed,trav", BLOCKED_LAUNCHES)
def test_sure_drops(ctx, sl, oracle, deck_seed, trav):
    """two keys of the launch behind 64 fillers each: every visit to them is dropped, reads a zero row and adds nothing, in the walk (fm_claim) as in the
    prefix replay (fm_find; for traverser 1 the blocked opponent key is the root, in the prefix of every cut > 0), and everything else is as the restatement
    with the two keys absent has it"""
    fx = blocked_launch(oracle, deck_seed, trav)
    rows, nb = fx.rows, 8
    assert rows.dropped > 0 and (rows.choice, rows.terminal) == (fx.base.choice, fx.base.terminal)
    h, _ = solver_of(ctx, sl, oracle, deck_seed, 3, capacity_log2=C_BIG)
    for cut in (-1, 0, 1, 2, 3):
        what = f"deck {deck_seed}, traverser {trav}, cut {cut}, two keys blocked"
        h.reset()
        set_rows(h, fx.fill)
        h.cut(cut)
        c0 = h.counters()
        raises(sl, sl.SCOPA_ENOMEM, h.traverse, trav, 0, 0, nb)
        c1 = h.counters()
        assert c1["dropped"] - c0["dropped"] == rows.dropped, what
        assert (c1["choice_visits"] - c0["choice_visits"], c1["terminal_visits"] - c0["terminal_visits"]) == (rows.choice, rows.terminal), what
        assert c1["rows"] == 128 + len(rows.count), what
        assert_delta(Visible(h, fx.fill), rows, what)
        assert not np.isin(np.array(fx.blocked, np.uint64), h.delta_get()[0]).any(), what
        tab = h.tables_get()
        fill = np.isin(tab[0], fx.fill)
        assert_own_rows(tuple(x[fill] for x in tab), what)
        raises(sl, sl.SCOPA_ENOMEM, h.traverse, trav, 0, 0, nb)            # no reset: the same visits are dropped again, and reported again
        c2 = h.counters()
        assert (c2["dropped"] - c1["dropped"], c2["rows"]) == (rows.dropped, c1["rows"]), what
