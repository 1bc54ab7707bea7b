"""The single verifiers (rs_*_verify, rs_*_verify_level) are a batch of one of the body behind rs_*_verify_batch.  What a caller
of the single entry points relies on and no other test pins: the kernel's scalar load path for a primary input that is not
16-byte aligned, the text of the noise error and the untouched report beside it, and a key that no verification writes to.

Every report is compared for equality with the CPU's (tests.test_verify.expected_report through
tests.test_verify_batch.expected)."""
import ctypes as C

import pytest
import torch

from tests import test_verify as TV
from tests import test_verify_batch as TB

SCHEMES = ["groth16", "rinocchio"]


def offset_by_one_word(t):
    """a copy of t that starts one 8-byte word into a larger tensor: 8-byte aligned, not 16-byte aligned"""
    buf = torch.empty(t.numel() + 2, dtype=t.dtype, device=t.device)
    assert buf.data_ptr() % 16 == 0
    view = buf[1:1 + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 16 == 8
    return view


@pytest.mark.gpu
@pytest.mark.parametrize("scheme", SCHEMES)
def test_primary_input_that_is_not_16_byte_aligned(scheme):
    """three public inputs (tests.test_verify.hand_rows); members: accepted, one input slot changed, accepted, one input
    slot changed, accepted"""
    k = TB.io_system(scheme, "hand")
    assert k["cs"].n_inputs >= 3
    d = TB.OnDevice(scheme, k)
    on = d.put(k["members"])
    exps = [TB.expected(scheme, k["ctx"], k["cs"], k["vk"], x, p) for x, p, _ in k["members"]]
    assert [e["accepted"] for e in exps] == [True, True, False, False]
    assert all(sum(e["n_bad"]) == 1 for e in exps[2:])  # a single changed slot
    for (x, p), e in zip(on, exps):
        assert x.data_ptr() % 16 == 0
        aligned, shifted = d.single(x, p), d.single(offset_by_one_word(x), p)
        assert shifted == aligned
        TV.assert_report(shifted, e)
    idx = [0, 2, 1, 3, 0]
    primaries, proofs = torch.stack([on[i][0] for i in idx]), [on[i][1] for i in idx]
    fn = d.dev.groth16_verify_batch if scheme == "groth16" else d.dev.rinocchio_verify_batch
    aligned, shifted = fn(d.dvk, primaries, proofs), fn(d.dvk, offset_by_one_word(primaries), proofs)
    assert shifted == aligned and len(shifted) == 5
    for g, i in zip(shifted, idx):
        assert not g.noise_spent
        TV.assert_report(g.result, exps[i])
    d.dvk.close()


@pytest.mark.gpu
@pytest.mark.parametrize("element,flags,suffix", [(0, [0, 0, 0], " (element 0 of the batch)"), (2, [0, 1, 0], "")])
def test_noise_error_names_the_first_spent_limb_and_leaves_the_report(element, flags, suffix):
    """the guard's text (seal_ring.tcc:450-453): the first spent limb, and the element's index inside its run of non-EMPTY
    elements where that run is longer than one"""
    from ringsnark_amd import _lib
    from ringsnark_amd.device import _ptr
    c = TV.g16_case("toy", 6)
    ctx, cs, vk = c["ctx"], c["cs"], c["vk"]
    dev = TV.device_for("toy")
    dvk = dev.groth16_vk(dev.r1cs(cs), vk)
    spent = TV.budget_ladder(ctx, vk["sk"])[-1]
    budget = list(ctx.noise_budget(vk["sk"], spent))
    assert min(budget) == 0
    limb = budget.index(0)
    proof = dev.put(c["proof"])
    proof[element] = dev.put(spent)
    primary = dev.put(c["asg"][: cs.n_inputs])
    rep = _lib.VerifyReport()
    C.memset(C.addressof(rep), 0xA5, C.sizeof(rep))
    before = bytes(rep)
    rc = dev.lib.rs_groth16_verify(dev.h, dvk.h, _ptr(primary), _ptr(proof), (C.c_int * 3)(*flags), C.byref(rep), dev.stream())
    assert rc == _lib.RS_ERR_NOISE
    assert dev.lib.rs_last_error().decode() == "ciphertext #%d has remaining noise budget 0 <= 0%s" % (limb, suffix)
    assert bytes(rep) == before
    dvk.close()


@pytest.mark.gpu
@pytest.mark.parametrize("scheme", SCHEMES)
def test_no_state_of_one_verification_shows_in_the_next(scheme):
    """one key: a single verification rejected in the last slot of the last limb, an accepted one, then a batch"""
    k = TB.four_kinds(scheme, "toy", 6 if scheme == "groth16" else 9, scheme == "rinocchio")
    prm, ctx, cs, vk = k["prm"], k["ctx"], k["cs"], k["vk"]
    primary, proof, _ = k["members"][0]
    last = TB.one_slot_changed(prm, primary, 1, prm.L - 1, prm.N - 1)
    members = [(last, proof), (primary, proof), k["members"][1][:2], (last, proof), k["members"][3][:2]]
    exps = [TB.expected(scheme, ctx, cs, vk, x, p) for x, p in members]
    assert [e["accepted"] for e in exps] == [False, True, True, False, False]
    assert exps[0]["first"][1:3] == (prm.L - 1, prm.N - 1) and sum(exps[0]["n_bad"]) == 1
    d = TB.OnDevice(scheme, k)
    on = d.put(members)
    TV.assert_report(d.single(*on[0]), exps[0])
    TV.assert_report(d.single(*on[1]), exps[1])
    for order in ([1, 0, 2, 3, 4], [0, 1]):
        for g, i in zip(d.batch([on[i] for i in order]), order):
            assert not g.noise_spent
            TV.assert_report(g.result, exps[i])
    TV.assert_report(d.single(*on[1]), exps[1])
    TV.assert_report(d.single(*on[0]), exps[0])
    d.dvk.close()
