"""Hand-computed known answers for tests/flr_ref.py, the yardstick of the site FLR stage."""
import math

import numpy as np

import flr_ref

TABLE_DTYPE = np.dtype([("best_prob", "<f8"), ("best_psm", "<u4"), ("n_psm", "<u4"), ("n_confident", "<u4"), ("n_in_best", "<u4"),
                        ("best_ascore", "<f4"), ("reserved", "<u4")])
P32 = 4294967296


def _six():
    """slot 0: 0.75, slot 1: empty, slot 2: 1.0, slot 3: 0.75 (ties slot 0), slot 4: 0.0, slot 5: 0.5 and a decoy"""
    t = np.zeros(6, TABLE_DTYPE)
    t["best_prob"] = [0.75, 0.9, 1.0, 0.75, 0.0, 0.5]
    t["n_psm"] = [2, 0, 1, 1, 3, 1]
    t["n_in_best"] = [1, 0, 1, 0, 0, 1]
    cls = np.array([0, 0, 0, 0, 0, 1], np.uint8)
    return t, cls


def test_err():
    assert flr_ref.err(1.0) == 0
    assert flr_ref.err(0.0) == 2 ** 32
    assert flr_ref.err(math.nextafter(1.0, 0.0)) == 0            # 2^-53 * 2^32 truncates
    assert flr_ref.err(0.75) == 2 ** 30 and flr_ref.err(0.5) == 2 ** 31
    assert flr_ref.err(1.5) == 0


def test_six_slots_by_hand():
    t, cls = _six()
    rec, order, n_ranked = flr_ref.flr(t, cls)
    assert n_ranked == 5
    assert order.tolist() == [2, 0, 3, 5, 4, 1]                  # 1.0 | 0.75 0.75 (by slot) | 0.5 | 0.0 | the empty slot
    # cut            rank  decoys  err_sum                      flr              raw ratio
    # {2}              1     0     0                            0                0 / 1
    # {2, 0, 3}        3     0     2 * 2^30                     (1/2) / 3        0 / 3
    # {.., 5}          4     1     2^31 + 2^31                  1 / 4            1 / 3
    # {.., 4}          5     1     2^32 + 2^32                  2 / 5            1 / 4
    want = {2: (1, 0, 0, 0.0, 0.0), 0: (3, 0, P32 // 2, 0.5 / 3.0, 0.0), 3: (3, 0, P32 // 2, 0.5 / 3.0, 0.0),
            5: (4, 1, P32, 0.25, 0.25), 4: (5, 1, 2 * P32, 0.4, 0.25)}
    for s, w in want.items():
        assert tuple(rec[s].tolist()) == w, s
    assert rec[0].tobytes() == rec[3].tobytes()                   # a tie group shares its record
    assert rec[1].tobytes() == bytes(32)                          # not ranked: zero bytes
    ranked = order[:n_ranked]
    assert (np.diff(rec["flr"][ranked]) >= 0).all()              # flr does not decrease along the order
    assert (np.diff(rec["decoy_q"][ranked]) >= 0).all()          # decoy_q does not increase towards better sites
    assert rec["decoy_q"][5] == 0.25 < 1.0 / 3.0                 # the minimum over the wider cuts


def test_classes_and_the_flag():
    t, cls = _six()
    rec, order, n_ranked = flr_ref.flr(t)                         # no classes: every slot a target
    assert n_ranked == 5 and not rec["n_decoy"].any() and not rec["decoy_q"].any()
    cls[4] = 2                                                    # left out
    rec, order, n_ranked = flr_ref.flr(t, cls)
    assert n_ranked == 4 and order.tolist() == [2, 0, 3, 5, 1, 4] and rec[4].tobytes() == bytes(32)
    assert tuple(rec[5].tolist()) == (4, 1, P32, 0.25, 1.0 / 3.0)
    rec, order, n_ranked = flr_ref.flr(t, None, reported_only=True)
    assert n_ranked == 3 and order.tolist() == [2, 0, 5, 1, 3, 4]
    assert tuple(rec[0].tolist()) == (2, 0, P32 // 4, 0.125, 0.0) and tuple(rec[5].tolist()) == (3, 0, 3 * (P32 // 4), 0.25, 0.0)
    cls[0] = 3
    try:
        flr_ref.flr(t, cls)
    except ValueError:
        pass
    else:
        raise AssertionError("class byte 3 was accepted")
    rec, order, n_ranked = flr_ref.flr(t[:0])
    assert rec.size == 0 and order.size == 0 and n_ranked == 0
