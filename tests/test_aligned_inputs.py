"""Conditions on the sign-aligned worst-case inputs of tests/test_msm_worst_case.py (builders: tests/helpers.py).  CPU only:
these are statements about the inputs, not about the kernels -- without them a passing kernel test would say nothing."""
import numpy as np
import pytest

from oracle import oracle as O
from ringsnark_amd import params as P
from tests import helpers as H


@pytest.mark.parametrize("name", ["toy49", "n2048", "toy50", "n2048q50"])
def test_closed_form_equals_the_oracle_inner_product(name):
    """sum_d count_d target_d mod Q_j is what EncodingElem::inner_product gives on the aligned terms, bit for bit: ring
    elements, an all-KIND_ONE vector, a second key for the same rows, and (toy49, toy50) a slot-constant vector as expanded rows."""
    variants = (("poly", 0), ("one", 0), ("poly", 1), ("const", 0), ("const", 1)) if name in ("toy49", "toy50") else (("poly", 0),)
    for variant, key in variants:
        ctx, rings, encs, targets, T, kinds = H.aligned_case(name, variant, key)
        assert T == H.aligned_T(ctx.Q) and encs.shape == targets.shape == ctx.enc_shape(H.ALIGNED_D)
        idx = np.arange(T) % H.ALIGNED_D
        rows = np.repeat(rings[:, :, None], ctx.N, axis=2) if variant == "const" else rings
        exp, used = ctx.inner_product(encs[idx], np.ascontiguousarray(rows[idx]), None if kinds is None else kinds[idx], threads=0)
        assert used == T
        assert (H.closed_form(ctx, targets, T) == exp).all(), (name, variant, key)


def test_aligned_T_is_a_handful_of_accumulator_periods():
    """ceil(2^53 / (0.30 min Q - 2^20)) + margin: about 107 + 4 terms at 48 bits, 1707 + 4 at 44 bits."""
    assert H.aligned_T([(1 << 48) - 1, (1 << 49) - 1]) == 107 + 4
    assert H.aligned_T([1 << 44], margin=9) == 1707 + 9
    assert H.aligned_T([(1 << 50) - 27]) == 27 + 4
    for bits in (40, 44, 48, 49, 50):
        Q = (1 << bits) - 1
        T = H.aligned_T([Q])
        assert (T - 4) * (0.30 * Q - 2**20) >= 2**53 > (T - 5) * (0.30 * Q - 2**20)


@pytest.mark.parametrize("name", sorted(H.WORST_CASES))
def test_every_slab_of_every_case_leaves_the_exact_integers(name):
    """Per (limb, component, prime) slab of every GPU case, with the case's own T: every |target| <= 0.30 Q_j, one sign per
    slab, both signs in the call, and the never-reduced running sum beyond 2^53 at some position."""
    variants = (("poly", 0), ("one", 0), ("const", 0), ("poly", 1)) if name in ("toy49", "toy50") else (("poly", 0),)
    for variant, key in variants:
        ctx, rings, encs, targets, T, kinds = H.aligned_case(name, variant, key)
        assert H.check_aligned_inputs(ctx, targets, T) > 1.0
        signs = {H.aligned_sign(i, c, j) for i in range(ctx.L) for c in range(2) for j in range(ctx.K)}
        assert signs == {1, -1}
        for j, Q in enumerate(ctx.Q):  # canonical key words
            assert (encs[:, :, :, j] < np.uint64(Q)).all()


def test_aligned_products_are_the_targets():
    """ct u = target (mod Q_j) at every position, with u recomputed from the rows through the oracle: ring elements, a group
    of two vectors (the spectrum of the summed lifts), KIND_ONE and slot-constant terms."""
    ctx = H.oracle_ctx(P.preset("toy49"))
    D = 3
    group = [ctx.random_ring(71, D), ctx.random_ring(72, D)]
    kinds = np.array([0, O.KIND_ONE, 0], dtype=np.uint8)
    for rings, kw in ((None, {}), (group, {}), (None, dict(kinds=kinds)), (None, dict(slot_const=True))):
        out_rings, encs, targets = H.aligned_terms(ctx, D, 5, rings=rings, **kw)
        vecs = rings if rings is not None else [out_rings]
        for d in range(D):
            for i in range(ctx.L):
                for j, Q in enumerate(ctx.Q):
                    u = np.zeros(ctx.N_enc, dtype=object)
                    for v in vecs:
                        u = u + H.term_spectra(ctx, v[d:d + 1], kw.get("kinds", [0] * D)[d:d + 1], kw.get("slot_const", False))[0, i, j].astype(object)
                    for c in range(2):
                        assert ((encs[d, i, c, j].astype(object) * u - targets[d, i, c, j]) % Q == 0).all(), (d, i, c, j)


@pytest.mark.parametrize("name", sorted(H.EXTREME_CASES))
def test_keys_aligned_to_groups_of_extreme_rows_leave_the_exact_integers(name):
    """The aligned key for a group of extreme rows: the same conditions, and on the smallest context the closed form
    against the oracle (enc_add across the group's vectors)."""
    ctx, rings, n_vecs, encs, targets, T = H.extreme_case(name)
    assert H.check_aligned_inputs(ctx, targets, T) > 1.0
    if name == "n8192":
        idx = np.arange(T) % H.ALIGNED_D
        one = ctx.inner_product(encs, np.ascontiguousarray(rings[idx]), threads=0, window=H.ALIGNED_D)[0]
        exp = one
        for _ in range(n_vecs - 1):
            exp = ctx.enc_add(exp, one)
        assert (H.closed_form(ctx, targets, T) == exp).all()


@pytest.mark.parametrize("name", ["n8192", "hybrid8192"])
def test_extreme_rows_round_trip_and_sit_at_the_ends_of_the_balanced_range(name):
    """batch_encode(extreme_rows(...)) is the polynomial asked for, and every centred lift has magnitude (q - 1) / 2, for a
    43-bit and a 54-bit ring prime at N = N_enc = 8192; the four patterns differ."""
    ctx = H.oracle_ctx(H.worst_case_params(name))
    q, seen = ctx.q[0], []
    for pattern in H.EXTREME_PATTERNS:
        rows = H.extreme_rows(ctx, 0, pattern, seed=3)
        assert rows.shape == (ctx.N,) and (rows < np.uint64(q)).all()
        lift = H.centred_lift(ctx.batch_encode(0, rows), q)
        assert (np.abs(lift) == (q - 1) // 2).all(), pattern
        if pattern == "plus":
            assert (lift > 0).all()
        elif pattern == "minus":
            assert (lift < 0).all()
        elif pattern == "alternating":
            assert (lift[0::2] > 0).all() and (lift[1::2] < 0).all()
        else:
            assert (lift > 0).any() and (lift < 0).any()
        seen.append(lift)
    assert len({s.tobytes() for s in seen}) == 4
