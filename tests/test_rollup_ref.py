"""tests/rollup_ref.py, the yardstick of the site roll-up, on hand-worked cases (no device)."""
import numpy as np

import rollup_ref
from pyascore_amd import _lib

SP = np.dtype(_lib.SITE_PROB_DTYPE)
PP = np.dtype(_lib.PSM_PROB_DTYPE)
NO = _lib.PYA_ROLLUP_NO_PSM
INF = np.float32(np.inf)


def _batch(psms):
    """psms: (kind, best_sig, [with_prob per residue], [ascores])"""
    n = len(psms)
    off = np.concatenate([[0], np.cumsum([len(p[2]) for p in psms])]).astype(np.int64)
    sp = np.zeros(int(off[-1]), SP)
    sp["with_prob"] = [w for p in psms for w in p[2]]
    sp["without_prob"] = 1.0 - sp["with_prob"]
    pp = np.zeros(n, PP)
    pp["kind"] = [p[0] for p in psms]
    sig = np.array([p[1] for p in psms], np.uint64)
    max_k = max(1, max(len(p[3]) for p in psms))
    asc = np.zeros((n, max_k), np.float32)
    for i, p in enumerate(psms):
        asc[i, :len(p[3])] = p[3]
    return sp, pp, off, sig, asc


def _row(t, s):
    r = t[s]
    return (float(r["best_prob"]), int(r["best_psm"]), int(r["n_psm"]), int(r["n_confident"]), int(r["n_in_best"]), float(r["best_ascore"]),
            int(r["reserved"]))


def test_hand_worked_table():
    psms = [
        (1, 0b01, [0.9, 0.1], [20.0]),           # PSM 0: residue 0 modified
        (1, 0b10, [0.25, 0.75], [7.5]),          # PSM 1: residue 1 modified; 0.75 meets the threshold exactly
        (1, 0b01, [0.9, 0.1], [INF]),            # PSM 2: ties PSM 0 on slot 0, Ascore +inf
        (2, 0b01, [-1.0, -1.0], [3.0]),          # PSM 3: OVER -- contributes nothing
        (1, 0b00, [0.0, 0.0], []),               # PSM 4: n_of_mod == 0 -- covers the slots, reports none
        (0, 0, [0.0, 0.0], []),                  # PSM 5: NONE
    ]
    sp, pp, off, sig, asc = _batch(psms)
    slot = np.array([0, 1, 0, 1, 0, -1, 0, 1, 0, 1, 0, 1], np.int32)       # PSM 2's second record is left out
    t = rollup_ref.table(sp, pp, off, sig, asc, slot, 3, 0.75)
    assert _row(t, 0) == (0.9, 0, 4, 2, 2, float("inf"), 0)
    assert _row(t, 1) == (0.75, 1, 3, 1, 1, 7.5, 0)
    assert _row(t, 2) == (0.0, NO, 0, 0, 0, 0.0, 0)                          # nobody covers it: the empty slot
    assert t.tobytes() != np.zeros(3, rollup_ref.DTYPE).tobytes() and rollup_ref.empty(3)[2].tobytes() == t[2].tobytes()
    # the smallest id among the ties, whatever the numbering
    ids = np.array([50, 40, 30, 20, 10, 0], np.uint32)
    t2 = rollup_ref.table(sp, pp, off, sig, asc, slot, 3, 0.75, psm_id=ids)
    assert _row(t2, 0)[1] == 30 and _row(t2, 1)[1] == 40
    t2["best_psm"] = t["best_psm"]
    assert t2.tobytes() == t.tobytes()                                       # ... and nothing else moves
    assert _row(rollup_ref.table(sp, pp, off, sig, asc, slot, 3, 0.75, psm_base=100), 0)[1] == 100


def test_two_records_of_one_psm_on_one_slot_and_slots_outside_the_table():
    sp, pp, off, sig, asc = _batch([(1, 0b11, [0.6, 0.8], [4.0, 9.0]), (1, 0b10, [0.1, 0.8], [2.0])])
    t = rollup_ref.table(sp, pp, off, sig, asc, np.array([0, 0, 5, 0], np.int32), 1, 0.7)
    assert _row(t, 0) == (0.8, 0, 3, 2, 3, 9.0, 0)                           # PSM 0 twice; PSM 1's slot 5 is outside
    t = rollup_ref.table(sp, pp, off, sig, asc, np.array([0, 0, 5, 0], np.int32), 6, 0.7)
    assert _row(t, 5) == (0.1, 1, 1, 0, 0, 0.0, 0)


def test_ascore_order_and_zero_probabilities():
    """negative Ascores are a max among themselves, lose to any non-negative one, and are not mistaken for the empty 0; a slot
    whose records all have probability 0 still names its smallest PSM"""
    sp, pp, off, sig, asc = _batch([(1, 1, [0.0], [-3.0]), (1, 1, [0.0], [-1.5]), (1, 1, [0.0], [-8.0])])
    t = rollup_ref.table(sp, pp, off, sig, asc, np.zeros(3, np.int32), 1, 0.75, psm_id=np.array([9, 4, 6], np.uint32))
    assert _row(t, 0) == (0.0, 4, 3, 0, 3, -1.5, 0)
    sp, pp, off, sig, asc = _batch([(1, 1, [0.5], [-3.0]), (1, 1, [0.5], [0.0])])
    assert _row(rollup_ref.table(sp, pp, off, sig, asc, np.zeros(2, np.int32), 1, 0.0), 0) == (0.5, 0, 2, 2, 2, 0.0, 0)
    keys = [rollup_ref.ascore_key(np.float32(x).view(np.uint32)) for x in (-np.inf, -2.0, -0.0, 0.0, 1e-30, 2.0, np.inf)]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)


def test_accumulation_equals_one_call_in_either_order():
    rng = np.random.default_rng(5)
    psms = []
    for _ in range(40):
        ns = int(rng.integers(1, 5))
        sig = int(rng.integers(0, 1 << ns))
        k = bin(sig).count("1")
        psms.append((int(rng.choice([1, 1, 1, 2, 0])), sig, rng.choice([0.0, 0.25, 0.5, 0.75, 1.0], ns).tolist(),
                     rng.choice([-2.0, 0.0, 3.0, 3.0, np.inf], k).astype(np.float32).tolist()))
    sp, pp, off, sig, asc = _batch(psms)
    slot = rng.integers(-1, 7, int(off[-1])).astype(np.int32)
    whole = rollup_ref.table(sp, pp, off, sig, asc, slot, 6, 0.75)
    assert whole["n_psm"].sum() > 20 and (whole["best_psm"] != NO).any()
    cut, rec = 17, int(off[17])
    halves = [(sp[:rec], pp[:cut], off[:cut + 1], sig[:cut], asc[:cut], slot[:rec], 0),
              (sp[rec:], pp[cut:], off[cut:] - rec, sig[cut:], asc[cut:], slot[rec:], cut)]
    for order in ((0, 1), (1, 0)):
        t = None
        for h in order:
            a = halves[h]
            t = rollup_ref.table(*a[:6], 6, 0.75, psm_base=a[6], into=t)
        assert t.tobytes() == whole.tobytes(), order
    from pyascore_amd import rollup as ru
    a, b = (rollup_ref.table(*h[:6], 6, 0.75, psm_base=h[6]) for h in halves)
    assert ru.merge(a, b).tobytes() == whole.tobytes() and ru.merge(b, a).tobytes() == whole.tobytes()
