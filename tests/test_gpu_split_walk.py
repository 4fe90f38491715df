"""The split walk of the fused score-localize body (csrc/fused_core.hip.h, walk_record_split): with both directions, charge 1,
at most 21 site assignments, L - 1 >= 6 and mz_error <= 0.49, one helper lane per site assignment walks the first
x = (L - 1) / 3 steps of both directions and the walker lanes the rest.  Every case below is compared bit for bit in best_score,
best_sig, n_sig, ascores and alt_mask against the reference's own core AND against the same scorer with PYA_DEBUG bit
0x08000000 ("no split walk") set, through the batch kernel (PYA_NO_TINY) and through the single-launch kernel (no switch, up
to 64 PSMs).

Shapes: L - 1 around the gate and the changes of x; peptides around the 32-step mask word; the numbers of site assignments at
the layout's edges; ion types with and without a subtracted offset and of one direction; the tolerance that keeps the old walk;
fixed modifications in a batch that mixes splitting and non-splitting PSMs; the hand-over to the general localize kernel.

Two departures from the list the cases were drawn from, both forced by the inputs themselves:
  * 22 and 32 sites do not fit a peptide of 20 residues: those two shapes run at L = 22 / L = 32 (every residue a site) and at
    L = 40, the others at L = 20 and L = 40.
  * peptides above 64 residues (L = 97, 98, 100: the general kernel takes them whole) are compared with the checker in every
    array but alt_mask, whose batch form packs residues into 64 bits (tests/test_gpu_general_edges.py, _keys); the two GPU runs
    are still compared in all five.
Every case must hold a non-zero Ascore (checked on the checker's results), so none passes on empty work."""
import numpy as np
import pytest

from conftest import checker_kind
from oracle import harness, orc
from pyascore_amd import synth
from test_gpu_general_edges import _same_results

pytestmark = pytest.mark.gpu

KEYS = ("best_score", "best_sig", "n_sig", "ascores", "alt_mask")
NO_SPLIT = 0x08000000
N_PSM = 96                       # per case: more than one single-launch batch, well under a second of checker time

# name -> (L, n_sites, n_mod, mz_error, fragment_types)
CASES = {}
for _L in (6, 7, 8, 9, 10):                                  # x = 0 (old walk), 2, 2, 2, 3; (L - 1) % 3 = 2, 0, 1, 2, 0
    CASES["gate_L%d" % _L] = (_L, 4, 2, 0.05, "by")
for _L in (33, 34, 49, 64, 97, 98, 100):                     # the mask word changes after 32 steps
    CASES["word_L%d" % _L] = (_L, 3, 1, 0.05, "by")
for _ns, _k, _Ls in ((2, 1, (20, 40)), (6, 3, (20, 40)), (7, 2, (20, 40)), (22, 1, (22, 40)), (32, 1, (32, 40))):
    for _L in _Ls:                                           # 2, 20, 21 (the last that splits), 22, 32 site assignments
        CASES["n_%d_%d_L%d" % (_ns, _k, _L)] = (_L, _ns, _k, 0.05, "by")
CASES["ions_cz"] = (20, 6, 3, 0.05, "cz")                    # an offset is subtracted: the other instantiation of the step loop
CASES["ions_b"] = (20, 6, 3, 0.05, "b")                      # one direction: untouched
CASES["err_0.5"] = (20, 6, 3, 0.5, "by")                     # half_check: the old walk
# ("by" at 0.05: n_6_3_L20)

_made = {}


def _case(name):
    """(settings, batch, the checker's results); made once"""
    if name not in _made:
        L, ns, k, err, types = CASES[name]
        batch, settings = synth.make_batch("cfg2", n_psm=N_PSM, seed=1000 + list(CASES).index(name), L=L, n_sites=ns, n_mod=k, mz_error=err,
                                           fragment_types=types)
        _made[name] = (settings, batch, _checker(settings, batch))
    return _made[name]


def _checker(settings, batch):
    return harness.make_scorer(orc.OracleAscore, settings, kind=checker_kind()).score_batch(batch, int(batch["n_of_mod"].max()))


def _gpu(settings, tiny, debug=0):
    from pyascore_amd import PyAscore
    gpu = harness.make_scorer(PyAscore, settings)
    gpu.reload_env()                                         # (every switch at its production default)
    if not tiny:
        gpu.set_debug("PYA_NO_TINY", "1")
    if debug:
        gpu.set_debug("PYA_DEBUG", str(debug))
    return gpu


def _keys_vs_checker(batch):
    return KEYS if int(np.diff(batch["pep_off"]).max()) <= 64 else tuple(k for k in KEYS if k != "alt_mask")


def _head(res, n):
    return {k: res[k][:n] for k in KEYS}


def _check(settings, batch, want, what, extra_debug=0):
    assert np.any(want["ascores"] != 0.0), "%s: no PSM with a non-zero Ascore" % what
    # the batch kernels
    split = _gpu(settings, False, extra_debug).score_batch(batch)
    plain = _gpu(settings, False, extra_debug | NO_SPLIT).score_batch(batch)
    _same_results(split, want, _keys_vs_checker(batch), what + " (batch kernel) against the checker")
    _same_results(split, plain, KEYS, what + " (batch kernel) against no split walk")
    # the single-launch kernel: at most 64 PSMs and no switch
    n = min(64, int(batch["n_psm"]))
    head = synth.slice_batch(batch, 0, n)
    assert np.any(want["ascores"][:n] != 0.0), "%s: no PSM with a non-zero Ascore among the first %d" % (what, n)
    split1 = _gpu(settings, True, extra_debug).score_batch(head)
    plain1 = _gpu(settings, True, extra_debug | NO_SPLIT).score_batch(head)
    _same_results(split1, _head(want, n), _keys_vs_checker(batch), what + " (single launch) against the checker")
    _same_results(split1, plain1, KEYS, what + " (single launch) against no split walk")


@pytest.mark.parametrize("name", list(CASES))
def test_split_walk_matches_the_reference_and_the_plain_walk(name):
    settings, batch, want = _case(name)
    _check(settings, batch, want, name)


def _mixed(n_each, seed):
    """splitting and non-splitting PSMs in one launch, every PSM with a fixed modification (n_aux > 0)"""
    parts = []
    for j, (L, ns, k) in enumerate(((20, 6, 3), (7, 4, 2), (6, 4, 2), (40, 22, 1), (33, 3, 1), (49, 3, 1), (20, 7, 2), (10, 4, 2))):
        b, settings = synth.make_batch("cfg2", n_psm=n_each, seed=seed + j, L=L, n_sites=ns, n_mod=k)
        # carbamidomethyl-sized shift on a residue in the middle (odd PSMs: a second one on the N-terminus, position 0)
        n_aux = 1 + (np.arange(n_each) & 1)
        b["aux_off"] = np.concatenate([[0], np.cumsum(n_aux)]).astype(np.int64)
        pos = np.zeros(int(n_aux.sum()), np.uint32)
        pos[b["aux_off"][:-1]] = 1 + L // 2
        b["aux_pos"] = pos
        b["aux_mass"] = np.where(pos > 0, 57.021465, 42.010565).astype(np.float32)
        parts.append(b)
    return settings, synth.concat_batches(parts)


def test_mixed_launch_with_fixed_modifications():
    settings, batch = _mixed(24, 2000)                       # 192 PSMs
    _check(settings, batch, _checker(settings, batch), "mixed shapes with fixed modifications")
    settings, batch = _mixed(8, 3000)                        # 64 PSMs: all eight shapes in one single-launch batch
    _check(settings, batch, _checker(settings, batch), "mixed shapes with fixed modifications, 64 PSMs")


def test_hand_over_from_the_split_walk():
    """PYA_DEBUG bit 512: the fused kernel declines every PSM after its walk; the count records and scores it leaves must
    give the reference's results through the general localize kernel"""
    settings, batch, want = _case("n_6_3_L20")
    _check(settings, batch, want, "hand-over (PYA_DEBUG 512)", extra_debug=512)
