"""What the verifiers launch, pinned to what they launched BEFORE the single and the batched verifier were merged into one
body per scheme.

tests/golden/verify_launches.json was recorded with `record()` below on the library of the commit before that merge and is
not regenerated from the code under test: a count that differs means that the merged body enqueues another kernel sequence
than the body it replaced.  Per case the whole map `kernel name -> launches` of ONE call (after one warm-up call of the same
shape, so that what a context builds once -- the decode constants of the level -- is not in it) is compared.  A single call
decodes once per run of non-EMPTY elements and checks once; a batch decodes once per run of its flattened elements.  Keys and
proofs are the toy cases of tests/test_verify.py; every member of a batch is the same proof with the same flags."""
import json
import os

import pytest

from tests import test_verify as TV
from tests.test_batch import launches

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "verify_launches.json")
# EMPTY flags that split the elements of a proof into two runs
SPLIT = {"groth16": [0, 1, 0], "rinocchio": [0, 0, 0, 0, 1, 0, 0, 0, 0]}
CALLS = [(scheme, B, split) for scheme in ("groth16", "rinocchio") for B in (0, 1, 3, 5) for split in (False, True)]  # B = 0: the single verifier


def call_id(scheme, B, split):
    return "%s, %s, %s" % (scheme, "single" if B == 0 else "batch of %d" % B, "two runs per proof" if split else "no EMPTY element")


def open_keys():
    """scheme -> (device, key, primary input, proof)"""
    out = {}
    for scheme in ("groth16", "rinocchio"):
        c = TV.g16_case("toy", 6) if scheme == "groth16" else TV.rin_case("toy", 6, True)
        dev = TV.device_for("toy")
        dvk = (dev.groth16_vk if scheme == "groth16" else dev.rinocchio_vk)(dev.r1cs(c["cs"]), c["vk"])
        out[scheme] = (dev, dvk, dev.put(c["asg"][: c["cs"].n_inputs]), dev.put(c["proof"]))
    return out


@pytest.fixture(scope="module")
def on_device():
    out = open_keys()
    yield out
    for _, dvk, _, _ in out.values():
        dvk.close()


def record_launches(on, scheme, B, split):
    dev, dvk, primary, proof = on[scheme]
    flags = SPLIT[scheme] if split else None
    if B == 0:
        single = dev.groth16_verify if scheme == "groth16" else dev.rinocchio_verify
        fn = lambda: single(dvk, primary, proof, flags)
    else:
        batch = dev.groth16_verify_batch if scheme == "groth16" else dev.rinocchio_verify_batch
        fn = lambda: batch(dvk, [primary] * B, [proof] * B, None if flags is None else [flags] * B)
    fn()
    return launches(dev, fn)


def record():
    on = open_keys()
    return {call_id(*c): record_launches(on, *c) for c in CALLS}


@pytest.fixture(scope="module")
def golden():
    return json.load(open(FIXTURE))


@pytest.mark.gpu
@pytest.mark.parametrize("scheme,B,split", CALLS, ids=[call_id(*c) for c in CALLS])
def test_verifier_launches_what_it_launched_before_the_merge(golden, on_device, scheme, B, split):
    exp = golden[call_id(scheme, B, split)]
    assert exp and record_launches(on_device, scheme, B, split) == exp
