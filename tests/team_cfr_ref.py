"""Float64 numpy restatement of the Team MiniScopa solver (scopa_team_cfr.hip): the level-ordered CFR sweep with weights, the value passes, and
the map between the reference's information-state strings and table rows.

TEST INFRASTRUCTURE, written for this repository's tests.  The rules come from the oracle's TeamState (oracle/oracle.py); the sweep is anchored to
the reference's own CFRTrainer._cfr_recursive by tests/golden/team_cfr.npz (tests/test_team_cfr_ref.py), and the GPU kernels are held to it bit for
bit.  Every float64 operation is one numpy elementwise operation (one rounding, no fused multiply-add), in the reference's order:

  reach     the running product from the root down, the mover's reach times its stored local_strategy (vanilla_cfr.py:83-85)
  value     np.sum(local_strategy * action_utils): the products added left to right (:87)
  update    traverser's rows only: regret_sum += opp_reach * (action_utils - value); strategy_sum += reach * local_strategy (:93-95); with weights
            (pos, neg, strat):  R <- R + dR;  R <- !(R <= 0) ? R * pos : R * neg;  S <- (S + dS) * strat.  weights None = no multiplication at all
  sigma     every row: positive regrets `!(R <= 0) ? R : 0` summed left to right, divided; uniform where the sum is not > 0 (:23-30, :97)

Shape: ply k is played by seat k & 3 (team (k & 3) >> 1) from a hand of 4 - (k >> 2) cards; depths 0..11 are choice nodes, 12..15 forced.  A Ref covers
the subtree below a root given as (perm, path of legal-action indices, reaches): its rows are level-major within the subtree, children of node j of
depth d at j * b + c.  For the empty path these are the library's rows.  Every history is its own infoset, so a row has one node.
"""
import ctypes as C
import re

import numpy as np

import oracle as O

N_CHOICE_DEPTHS = 12
WIDTH = [1, 4, 16, 64, 256, 768, 2304, 6912, 20736, 41472, 82944, 165888, 331776]
OFFSET = [0, 1, 5, 21, 85, 341, 1109, 3413, 10325, 31061, 72533, 155477, 321365]
N_CHOICE, N_LEAVES, N_INFOSETS = 321365, 331776, 321365 + 4 * 331776


def branch(d):
    return 4 - (d >> 2) if d < 16 else 0


def team_of(d):
    return (d & 3) >> 1


def path_index(path):
    """mixed-radix index of a path of legal-action indices within its level, first ply most significant (forced plies contribute nothing)"""
    idx = 0
    for d, c in enumerate(path[:N_CHOICE_DEPTHS]):
        idx = idx * branch(d) + int(c)
    return idx


_LEAVES = {}


def leaves(perm):
    """int8 [331776]: reward x2 of team 0 at every depth-12 node (after its four forced plies), by the oracle's rules; enumerated once per deal and session"""
    key = bytes(np.ascontiguousarray(perm, np.uint8))
    if key in _LEAVES:
        return _LEAVES[key]
    L = O.lib()
    out = np.zeros(N_LEAVES, np.int8)
    buf = (C.c_int * 4)()
    root = O.TeamState(perm=np.frombuffer(key, np.uint8)).s
    cls = type(root)

    def rec(s, d, idx):
        n = L.ogt_legal(C.byref(s), buf)
        acts = buf[:n]
        if d == N_CHOICE_DEPTHS:
            t = cls.from_buffer_copy(s)
            for _ in range(4):
                L.ogt_legal(C.byref(t), buf)
                L.ogt_step(C.byref(t), buf[0])
            assert t.terminal
            out[idx] = t.r2[0]
            return
        assert n == branch(d)
        for c, a in enumerate(acts):
            t = cls.from_buffer_copy(s)
            L.ogt_step(C.byref(t), a)
            rec(t, d + 1, idx * n + c)

    rec(root, 0, 0)
    out.setflags(write=False)
    _LEAVES[key] = out
    return out


def state_at(perm, path):
    """the oracle's TeamState after the legal-action indices of `path`"""
    s = O.TeamState(perm=perm)
    for c in path:
        s.step(s.legal()[int(c)])
    return s


def key_to_path(perm, key):
    """information-state string -> path of legal-action indices, or None when the string is not the key of a node of this deal"""
    m = re.fullmatch(r"Team([01]):P([0-3]):H\[[^\]]*\]:T\[[^\]]*\]:A\[([0-9-]*)\]", key)
    if not m:
        return None
    acts = [int(x) for x in m.group(3).split("-")] if m.group(3) else []
    if len(acts) > 15:
        return None
    s, path = O.TeamState(perm=perm), []
    for a in acts:
        legal = s.legal()
        if a not in legal:
            return None
        path.append(legal.index(a))
        s.step(a)
    return tuple(path) if s.infoset_string(s.current_player()) == key else None


def path_to_key(perm, path):
    s = state_at(perm, path)
    return s.infoset_string(s.current_player())


def dfs_preorder(d0=0):
    """The reference's dict insertion order below a depth-d0 root (first visit = DFS pre-order, vanilla_cfr.py:74-85), as
    (rows, forced): rows = the subtree-local row of every choice node in that order; forced = (local depth-12 index, depth) of every forced node."""
    off, o = {}, 0
    for d in range(d0, N_CHOICE_DEPTHS):
        off[d] = o
        o += WIDTH[d] // WIDTH[d0]
    rows, forced = [], []

    def rec(d, idx):
        if d >= N_CHOICE_DEPTHS:
            for k in range(d, 16):
                forced.append((idx, k))
            return
        rows.append(off[d] + idx)
        for c in range(branch(d)):
            rec(d + 1, idx * branch(d) + c)

    rec(d0, 0)
    return np.array(rows, np.int64), np.array(forced, np.int64)


def dfs_paths(limit=None):
    """paths of the whole tree's nodes (forced ones included) in DFS pre-order, as a generator"""
    stack = [()]
    n = 0
    while stack:
        p = stack.pop()
        yield p
        n += 1
        if limit is not None and n >= limit:
            return
        d = len(p)
        if d < 15:
            for c in reversed(range(max(branch(d), 1) if d < N_CHOICE_DEPTHS else 1)):
                stack.append(p + (c,))


FOLLOW, UNIFORM, MAXIMISE = 0, 1, 2


class Ref:
    def __init__(self, perm, path=(), reaches=(1.0, 1.0)):
        self.perm = np.ascontiguousarray(perm, np.uint8)
        self.d0 = len(path)
        assert self.d0 <= N_CHOICE_DEPTHS - 1
        self.reaches = (float(reaches[0]), float(reaches[1]))
        self.width = {d: WIDTH[d] // WIDTH[self.d0] for d in range(self.d0, 13)}
        self.off, o = {}, 0
        for d in range(self.d0, N_CHOICE_DEPTHS):
            self.off[d] = o
            o += self.width[d]
        self.n_rows, self.n_leaves = o, self.width[12]
        i0 = path_index(path)
        self.r2 = leaves(self.perm)[i0 * self.n_leaves:(i0 + 1) * self.n_leaves].astype(np.int64)

    def rows(self, d):
        return slice(self.off[d], self.off[d] + self.width[d])

    def tables(self):
        """reset state: (regret, strategy, local) [n_rows][4], leaf_reach_sum [2][n_leaves]"""
        R, S, L = np.zeros((self.n_rows, 4)), np.zeros((self.n_rows, 4)), np.zeros((self.n_rows, 4))
        for d in range(self.d0, N_CHOICE_DEPTHS):
            L[self.rows(d), :branch(d)] = 1.0 / branch(d)
        return R, S, L, np.zeros((2, self.n_leaves))

    @staticmethod
    def sigma(R, b):
        """regret matching of rows R[:, :b] -> [n][4], zeros beyond b"""
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            pos = np.where(~(R[:, :b] <= 0.0), R[:, :b], 0.0)
            s = pos[:, 0].copy()
            for c in range(1, b):
                s = s + pos[:, c]
            out = np.zeros((R.shape[0], 4))
            out[:, :b] = np.where((s > 0.0)[:, None], pos / s[:, None], 1.0 / b)
        return out

    def traverse(self, R, S, L, Q, p, w=None):
        """one traversal of team p in place -> root value"""
        r = {self.d0: (np.array([self.reaches[0]]), np.array([self.reaches[1]]))}
        with np.errstate(invalid="ignore", over="ignore", under="ignore"):
            for d in range(self.d0, N_CHOICE_DEPTHS):
                b, sg = branch(d), L[self.rows(d), :branch(d)]
                r0, r1 = r[d]
                c0 = (r0[:, None] * sg) if team_of(d) == 0 else np.repeat(r0[:, None], b, 1)
                c1 = (r1[:, None] * sg) if team_of(d) == 1 else np.repeat(r1[:, None], b, 1)
                r[d + 1] = (c0.reshape(-1), c1.reshape(-1))
            q = Q[p] + r[12][p]
            Q[p] = q if w is None else q * float(w[2])
            val = 0.5 * (self.r2 if p == 0 else -self.r2).astype(np.float64)
            for d in range(N_CHOICE_DEPTHS - 1, self.d0 - 1, -1):
                b, rows = branch(d), self.rows(d)
                u, ls = val.reshape(-1, b), L[rows, :b].copy()
                prod = ls * u
                v = prod[:, 0].copy()
                for c in range(1, b):
                    v = v + prod[:, c]
                if team_of(d) == p:
                    reach, opp = r[d][p], r[d][1 - p]
                    Rn = R[rows, :b] + opp[:, None] * (u - v[:, None])
                    Sn = S[rows, :b] + reach[:, None] * ls
                    if w is not None:
                        Rn = np.where(~(Rn <= 0.0), Rn * float(w[0]), Rn * float(w[1]))
                        Sn = Sn * float(w[2])
                    R[rows, :b], S[rows, :b] = Rn, Sn
                L[rows] = self.sigma(R[rows], b)
                val = v
        return float(val[0])

    def iterate(self, R, S, L, Q, n_iters=None, weights=None):
        """iterations of "for p in (0, 1): traverse" in place -> root values [n][2]"""
        ws = [None] * n_iters if weights is None else list(np.asarray(weights, np.float64).reshape(-1, 3))
        out = np.zeros((len(ws), 2))
        for t, w in enumerate(ws):
            for p in (0, 1):
                out[t, p] = self.traverse(R, S, L, Q, p, w)
        return out

    def average_policy(self, S):
        """InfoNode.policy (vanilla_cfr.py:32-39) of every row"""
        out = np.zeros((self.n_rows, 4))
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            for d in range(self.d0, N_CHOICE_DEPTHS):
                b, rows = branch(d), self.rows(d)
                s = S[rows, 0].copy()
                for c in range(1, b):
                    s = s + S[rows, c]
                out[rows, :b] = np.where((s > 0.0)[:, None], S[rows, :b] / s[:, None], 1.0 / b)
        return out

    def value_pass(self, modes, tabs, persp, want_table=False):
        """one upward pass; modes / tabs per team; values are team `persp`'s.  -> (root value, table played or None)"""
        out = np.zeros((self.n_rows, 4)) if want_table else None
        val = 0.5 * (self.r2 if persp == 0 else -self.r2).astype(np.float64)
        with np.errstate(invalid="ignore", over="ignore", under="ignore"):
            for d in range(N_CHOICE_DEPTHS - 1, self.d0 - 1, -1):
                b, rows, t = branch(d), self.rows(d), team_of(d)
                u = val.reshape(-1, b)
                if modes[t] == MAXIMISE:
                    key = u if t == persp else -u
                    best, kb = np.zeros(u.shape[0], np.int64), key[:, 0].copy()
                    for c in range(1, b):
                        better = key[:, c] > kb
                        best, kb = np.where(better, c, best), np.where(better, key[:, c], kb)
                    row = (np.arange(b)[None, :] == best[:, None]).astype(np.float64)
                    v = u[np.arange(u.shape[0]), best]
                else:
                    row = tabs[t][rows, :b] if modes[t] == FOLLOW else np.full((u.shape[0], b), 1.0 / b)
                    v = np.zeros(u.shape[0])
                    for c in range(b):
                        v = v + row[:, c] * u[:, c]
                if out is not None:
                    out[rows, :b] = row
                val = v
        return float(val[0]), out

    def exploitability(self, policy, want_tables=False):
        """-> ([(BR0 + BR1) / 2, BR0, BR1, value for team 0], [br table of team 0, of team 1] or None)"""
        b0, t0 = self.value_pass((MAXIMISE, FOLLOW), (policy, policy), 0, want_tables)
        b1, t1 = self.value_pass((FOLLOW, MAXIMISE), (policy, policy), 1, want_tables)
        v, _ = self.value_pass((FOLLOW, FOLLOW), (policy, policy), 0)
        return np.array([(b0 + b1) / 2.0, b0, b1, v]), ([t0, t1] if want_tables else None)

    def minimax(self, want_table=False):
        return self.value_pass((MAXIMISE, MAXIMISE), (None, None), 0, want_table)

    def policy_value(self, a=None, b=None):
        return self.value_pass((UNIFORM if a is None else FOLLOW, UNIFORM if b is None else FOLLOW), (a, b), 0)[0]

    # ---- info_set_map entries of the whole tree -------------------------------------------------------------------------------------------
    def info_node(self, path, R, S, L, Q):
        """(legal_actions, regret_sum, strategy_sum, local_strategy) of the node at `path`, as the reference's InfoNode holds them (whole tree only)"""
        assert self.d0 == 0
        d, s = len(path), state_at(self.perm, path)
        legal = np.array(s.legal())
        if d < N_CHOICE_DEPTHS:
            row, b = OFFSET[d] + path_index(path), branch(d)
            return legal, R[row, :b].copy(), S[row, :b].copy(), L[row, :b].copy()
        return legal, np.zeros(1), np.array([Q[team_of(d), path_index(path)]]), np.ones(1)
