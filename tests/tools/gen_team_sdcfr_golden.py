"""tests/golden/team_sdcfr.npz: the reference's own DeepCFR on TPIMiniScopaGame, one traversal per traverser.

TEST INFRASTRUCTURE, run by hand on a machine that holds the reference checkout (CPU only):

    python tests/tools/gen_team_sdcfr_golden.py [/path/to/reference]

It imports the reference's Python through oracle/refshim.py's stand-ins for pyspiel / pettingzoo / gymnasium, builds
DeepCFR(load_game("team_mini_scopa_tpi")) -- which runs unmodified on the team game: _state_to_features parses H[...] and T[...] of the information
state string and ignores A[...] -- loads the two advantage nets saved in tests/golden/sdcfr.npz and runs _external_sampling_cfr from the initial state
(the reference's default deal, seed 42) once per traverser.  Recorded per traverser t:

    perm                 the deal, uint8 [16], seat s at bytes 4 s .. 4 s + 3, card id = action id
    t{t}_draw_action     the card every np.random.choice call returned, in call order; t{t}_draw_options: how many cards it chose from; t{t}_draw_uniform:
                         1 where the call was the uniform fall-back (no p)
    t{t}_row_bits        uint32 per appended row: features[0..32) as bits (hand one-hot | table multi-hot << 16); features[32..34) are checked to be [1, 0]
    t{t}_row_mask        uint16 per appended row: the mask as bits
    t{t}_row_regret      float32 [rows][16]: the normalised regrets as stored
    t{t}_value           the root value (float64 of what the call returned); t{t}_value_is_f32
    t{t}_visits_by_depth non-terminal calls per depth [16]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle")]


def main(reference=None):
    import importlib
    import refshim
    refshim.import_reference(*([reference] if reference else []))
    import torch
    import pyspiel
    importlib.import_module("envs.openspiel_team_mini_scopa")
    dc = importlib.import_module("deep_cfr")
    game = pyspiel.load_game("team_mini_scopa_tpi")
    torch.manual_seed(0)
    np.random.seed(0)
    d = dc.DeepCFR(game, num_players=2, device="cpu")
    z = np.load(os.path.join(ROOT, "tests", "golden", "sdcfr.npz"))
    for p in range(2):
        d.advantage_nets[p].net.load_state_dict({str(k): torch.from_numpy(z[f"net{p}__{k}"]) for k in z[f"net{p}_names"]})
    s0 = game.new_initial_state()
    deck = importlib.import_module("envs.team_mini_scopa_game").MiniDeck
    card_id = lambda c: deck.suits.index(c.suit) * 4 + deck.ranks[c.suit].index(c.rank)
    perm = np.array([card_id(c) for pl in s0.env.game.players for c in pl.hand], np.uint8)
    assert sorted(perm.tolist()) == list(range(16))
    out = {"perm": perm}
    orig_choice, orig_feats = np.random.choice, d._state_to_features
    for trav in (0, 1):
        draws, depths = [], []

        def choice(a, size=None, replace=True, p=None):
            r = orig_choice(a, size=size, replace=replace, p=p)
            draws.append((int(r), len(a), 1 if p is None else 0))
            return r

        def feats(state, player):
            depths.append(len(state.action_history))
            return orig_feats(state, player)

        np.random.choice, d._state_to_features = choice, feats
        n_before = len(d.advantage_nets[trav].buffer)
        np.random.seed(100 + trav)
        try:
            val = d._external_sampling_cfr(game.new_initial_state(), trav)
        finally:
            np.random.choice, d._state_to_features = orig_choice, orig_feats
        rows = list(d.advantage_nets[trav].buffer)[n_before:]
        f = np.array([r[0] for r in rows], np.float32)
        m = np.array([r[2] for r in rows], np.float32)
        assert set(np.unique(f).tolist()) <= {0.0, 1.0} and np.all(f[:, 32] == 1.0) and np.all(f[:, 33] == 0.0)
        w = (1 << np.arange(32, dtype=np.uint64))
        out[f"t{trav}_row_bits"] = (f[:, :32].astype(np.uint64) * w).sum(1).astype(np.uint32)
        out[f"t{trav}_row_mask"] = (m.astype(np.uint64) * w[:16]).sum(1).astype(np.uint16)
        out[f"t{trav}_row_regret"] = np.array([r[1] for r in rows], np.float32)
        out[f"t{trav}_draw_action"] = np.array([a for a, _, _ in draws], np.int8)
        out[f"t{trav}_draw_options"] = np.array([n for _, n, _ in draws], np.int8)
        out[f"t{trav}_draw_uniform"] = np.array([u for _, _, u in draws], np.int8)
        out[f"t{trav}_value"] = np.array([float(val)])
        out[f"t{trav}_value_is_f32"] = np.array([isinstance(val, np.float32)])
        out[f"t{trav}_visits_by_depth"] = np.bincount(np.array(depths), minlength=16).astype(np.int64)
        print(f"team sdcfr trav {trav}: visits={len(depths)} rows={len(rows)} draws={len(draws)} value={float(val)!r} type={type(val).__name__}")
    path = os.path.join(ROOT, "tests", "golden", "team_sdcfr.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(*sys.argv[1:2])
