"""The device constants of a context (table descriptors, moduli) belong to that context alone: entry points that read
them -- batch encoding, encode / inner product / decode / noise budget, ring inverse, uniform fill -- give the oracle's
results on two contexts alive at once, after one of them is destroyed, on a context created where the destroyed one
was, and on every arithmetic (toy: FP64, toy60: integer, toy54: hybrid, toy forced to the integer arithmetic)."""
import numpy as np
import pytest

from ringsnark_amd import params as P
from tests import helpers as H

T = 3  # terms of the inner product
_EXPECTED = {}


def expected(name):
    """Oracle inputs and results of a preset, computed once and never modified."""
    if name not in _EXPECTED:
        prm = P.preset(name)
        ctx = H.oracle_ctx(prm)
        e = {"prm": prm}
        e["rings"] = ctx.random_ring(11, T)
        e["plain"] = np.stack([np.stack([ctx.batch_encode(i, e["rings"][t, i]) for i in range(ctx.L)]) for t in range(T)])
        e["sk"] = ctx.keygen(5)
        e["encs"] = ctx.enc_encode(e["sk"], e["rings"], 7)
        e["coeff"] = ctx.random_ring(13, T)
        e["ip"], used = ctx.inner_product(e["encs"], e["coeff"])
        assert used == T
        e["dec"] = ctx.enc_decode(e["sk"], e["ip"])
        want = ctx.ring_mul(e["rings"][0], e["coeff"][0])
        for t in range(1, T):
            want = ctx.ring_add(want, ctx.ring_mul(e["rings"][t], e["coeff"][t]))
        assert (e["dec"] == want).all()  # the decoding is the inner product of the ring elements
        e["budget"] = np.array(ctx.noise_budget(e["sk"], e["ip"]))
        assert e["budget"].min() > 0
        unit = ctx.random_ring(17)
        unit[unit == 0] = 1
        e["unit"] = unit
        e["non_unit"] = unit.copy()
        e["non_unit"][ctx.L - 1, ctx.N - 1] = 0
        e["one"] = ctx.ring_scalar(1)
        _EXPECTED[name] = e
    return _EXPECTED[name]


def step_batch_encode(dev, e, s):
    from ringsnark_amd.device import to_host
    assert (to_host(dev.batch_encode(dev.put(e["rings"]))) == e["plain"]).all()


def step_encode(dev, e, s):
    from ringsnark_amd.device import to_host
    s["sk"] = dev.put(e["sk"])
    s["encs"] = dev.enc_encode(s["sk"], dev.put(e["rings"]), 7)
    assert (to_host(s["encs"]) == e["encs"]).all()


def step_inner_product(dev, e, s):
    from ringsnark_amd.device import to_host
    s["ip"], used = dev.inner_product(s["encs"], dev.put(e["coeff"]))
    assert used == T and (to_host(s["ip"]) == e["ip"]).all()


def step_decode(dev, e, s):
    from ringsnark_amd.device import to_host
    assert (to_host(dev.enc_decode(s["sk"], s["ip"])) == e["dec"]).all()


def step_noise_budget(dev, e, s):
    assert (dev.enc_noise_budget(s["sk"], s["ip"])[0] == e["budget"]).all()


def step_ring_inv(dev, e, s):
    from ringsnark_amd import _lib
    from ringsnark_amd.device import to_host
    u = dev.put(e["unit"])
    assert (to_host(dev.ring_mul(dev.ring_inv(u), u)) == e["one"]).all()
    with pytest.raises(_lib.RsError) as ei:
        dev.ring_inv(dev.put(e["non_unit"]))
    assert ei.value.code == _lib.RS_ERR_NOT_INVERTIBLE


def step_fill_uniform(dev, e, s):
    from ringsnark_amd.device import to_host
    prm = e["prm"]
    ring = to_host(dev.fill_uniform(dev.ring_empty(2), 0, 99))
    for i, q in enumerate(prm.q):
        assert (ring[:, i] < np.uint64(q)).all()
    enc = to_host(dev.fill_uniform(dev.enc_empty(1), 1, 99))
    for j, Q in enumerate(prm.Q):
        assert (enc[:, :, :, j] < np.uint64(Q)).all()
    # beyond the ring primes where the moduli differ in size: the words of layout 1 were drawn against Q, not q
    if max(prm.Q) > 2 * max(prm.q):
        assert (enc.max(axis=(0, 1, 2, 4)) >= np.uint64(max(prm.q))).all()
    assert (to_host(dev.fill_uniform(dev.ring_empty(2), 0, 99)) == ring).all()
    assert (to_host(dev.fill_uniform(dev.enc_empty(1), 1, 99)) == enc).all()


STEPS = (step_batch_encode, step_encode, step_inner_product, step_decode, step_noise_budget, step_ring_inv, step_fill_uniform)


def run_interleaved(devs):
    """every step on every context in turn, so that each context's calls fall between the other's"""
    state = [{} for _ in devs]
    for step in STEPS:
        for (dev, name), s in zip(devs, state):
            step(dev, expected(name), s)


def destroy(dev):
    dev.lib.rs_ctx_destroy(dev.h)
    dev.h = None


@pytest.mark.gpu
def test_two_contexts_interleaved():
    from ringsnark_amd.device import Device
    a, b = Device(P.preset("toy")), Device(P.preset("toy60"))
    run_interleaved([(a, "toy"), (b, "toy60")])
    run_interleaved([(b, "toy60"), (a, "toy")])  # warm: every lazily built constant exists now


@pytest.mark.gpu
def test_context_lifetimes():
    from ringsnark_amd import _lib
    from ringsnark_amd.device import Device
    a, b = Device(P.preset("toy")), Device(P.preset("toy60"))
    run_interleaved([(a, "toy"), (b, "toy60")])
    destroy(a)
    run_interleaved([(b, "toy60")])
    c = Device(P.preset("toy54"))  # its address may be the destroyed context's
    run_interleaved([(c, "toy54"), (b, "toy60")])
    with _lib.tuning(force_int_arith=1):
        d = Device(P.preset("toy"))
        run_interleaved([(d, "toy"), (c, "toy54")])
    destroy(b)
    run_interleaved([(d, "toy"), (c, "toy54")])
