"""CPU restatement of the sampled best response of FullScopa over a set of decks (k_full_chance_respond, k_full_chance_harden in
scopa_amd/csrc/scopa_full_chance.hip; respond_traverse / respond_iterate / harden in include/scopa.h), built on tests/full_chance_ref.py.

TEST INFRASTRUCTURE.  Rows, root_on and wide_key are full_chance_ref's, and its `walk` is the model: the walk here is that walk with ONE difference,
at a node whose mover is not the responder.

  opponent  a FIXED policy outside the responder's rows: `opp` is None (uniform play) or anything with dicts R and S by pair (a Rows), read by
            `which`: 0 the rule of full_chance_ref.match (F.average_probs of opp.S: strategy / total where the pair is held and total > 1e-12, else
            uniform), 1 regret matching of opp.R, an absent pair a zero row.  Nothing of the responder's rows is touched or counted there.
  rows      at the responder's nodes the walk is full_chance_ref.walk: touch, sigma from the frozen regrets, dR / A / count
  draws     (state.step << 16 | q, traversal id, iteration, deck_index << 8 | 144 + responder)
  harden    S[key] = one-hot at the FIRST maximal regret over the key's action count; R untouched
Variant for the guards (test_full_chance_respond_ref.py): tag= puts another tag base in 144's place."""
import oracle as O
import full_chance_ref as X
import full_mccfr_ref as F

RESPOND_TAG = 144


def opp_probs(opp, which, key, n):
    """the fixed opponent's probabilities at a node of n > 1 slots"""
    if opp is None:
        return [1.0 / n] * n
    if which == 0:
        return F.average_probs(opp.S, key, n)                              # (the rule of full_chance_ref.match)
    return F.sigma_of(opp.R.get(key, [0.0] * 3), n)


def walk(st, resp, tid, iteration, seed, rows, deck_index, opp=None, which=0, q=0, tag=RESPOND_TAG):
    """one response traversal below `st` on the deck it carries: the value of `st` for the responder; increments into the responder's rows only"""
    s = st.s
    if s.terminal:
        rows.terminal += 1
        v = s.r2[0] / 2.0
        return -v if resp else v
    p = s.step & 1
    h = sorted(F.hand(st, p))
    n = len(h)
    if n == 1:
        return walk(F.child(st, h[0]), resp, tid, iteration, seed, rows, deck_index, opp, which, q, tag)
    key = X.wide_key(st, p)
    rows.choice += 1
    if p != resp:
        u = O.philox_uniform(seed, (int(s.step) << 16) | q, tid, iteration, (deck_index << 8) | (tag + resp))
        a = F.pick(opp_probs(opp, which, key, n), u)
        return walk(F.child(st, h[a]), resp, tid, iteration, seed, rows, deck_index, opp, which, q, tag)
    rows.touch(key)
    sigma = F.sigma_of(rows.R[key], n)
    cfv = [walk(F.child(st, h[a]), resp, tid, iteration, seed, rows, deck_index, opp, which, q * n + a, tag) for a in range(n)]
    v = 0.0
    for a in range(n):
        v += sigma[a] * cfv[a]
    for a in range(n):
        inc = cfv[a] - v
        rows.dR[key][a] += inc
        rows.A[key][a] += abs(inc)
    rows.count[key] += 1
    return v


def traverse(root, decks, resp, iteration, b0, nb, seed, rows, opp=None, which=0, listed=None, tag=RESPOND_TAG):
    """nb response traversals on each listed deck (None: all), deck-major as the launch numbers them"""
    for d in (range(len(decks)) if listed is None else listed):
        st = X.root_on(root, decks[d])
        for i in range(nb):
            walk(st, resp, (b0 + i) & 0xFFFFFFFF, iteration, seed, rows, int(d), opp, which, 0, tag)


def iterate(root, decks, batch, seed, rows, counter, opp=None, which=0, listed=None):
    """one iteration from the handle's counter: responder 0, apply, responder 1, apply over `listed` -> the counter after it"""
    for resp in range(2):
        traverse(root, decks, resp, counter, 0, batch, seed, rows, opp, which, listed)
        rows.apply()
        counter += 1
    return counter


def harden(rows):
    """every row's strategy becomes the pure policy of its regrets: 1.0 at the first maximal regret over the key's action count"""
    for key, R in rows.R.items():
        n = X.key_actions(key)
        best = 0
        for a in range(1, n):
            if R[a] > R[best]:
                best = a
        rows.S[key] = [1.0 if a == best else 0.0 for a in range(3)]


def regret_gap(rows):
    """(the smallest POSITIVE difference between the best and the second regret over the rows' legal slots, [(key, best slot, second slot)] of the
    rows whose two largest regrets are equal): how far a sum may move before an argmax flips, and the rows where any order of adds may flip it"""
    gap, ties = float("inf"), []
    for key, R in rows.R.items():
        n = X.key_actions(key)
        order = sorted(range(n), key=lambda a: (-R[a], a))
        d = R[order[0]] - R[order[1]]
        if d > 0.0:
            gap = min(gap, d)
        else:
            ties.append((key, order[0], order[1]))
    return gap, ties


def exact_regret(root, decks, resp, opp=None, which=0):
    """{(A, B): [3]} the counterfactual regret increment of every responder infoset when the responder plays uniformly (zero regrets) and the other
    player plays the fixed opponent, SUMMED over the decks by key: the expectation of one response traversal per deck from zero tables
    (full_chance_ref.exact_regret's recursion with the opponent's probabilities in the place of 1 / n)"""
    out = {}

    def rec(st, reach):
        s = st.s
        if s.terminal:
            v = s.r2[0] / 2.0
            return -v if resp else v
        p = s.step & 1
        h = sorted(F.hand(st, p))
        n = len(h)
        if n == 1:
            return rec(F.child(st, h[0]), reach)
        key = X.wide_key(st, p)
        if p != resp:
            prob = opp_probs(opp, which, key, n)
            return sum(pr * rec(F.child(st, c), reach * pr) for pr, c in zip(prob, h) if pr > 0.0)
        cfv = [rec(F.child(st, c), reach) for c in h]
        v = sum(cfv) / n
        row = out.setdefault(key, [0.0] * 3)
        for a in range(n):
            row[a] += reach * (cfv[a] - v)
        return v

    for deck in decks:
        rec(X.root_on(root, deck), 1.0)
    return out
