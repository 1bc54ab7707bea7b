"""What the provers launch, and the workspace a batched proof reserves, pinned to what they were BEFORE the single and the
batched provers were merged into one body per scheme.

tests/golden/prover_launches.json was recorded with `record()` below on the library of the commit before that merge and is
not regenerated from the code under test: a count that differs means that the merged body enqueues another kernel sequence
than the body it replaced.  Per case the whole map `kernel name -> launches` of ONE call (after one warm-up call of the same
shape, so that what a context builds once -- plans, the io cache, the plaintext of (1, .., 1) -- is not in it) is compared,
and rs_prove_batch_bytes for both schemes at batch 1, 2, 3 and 8.  Keys and members are those of tests/test_batch.py."""
import json
import os

import pytest

from tests.test_batch import batch_case, launches, prove_batch, stack_d
from tests.test_seeded import prove

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "prover_launches.json")
# label -> (batch_case arguments, tuning knobs of the call)
KEYS = {
    "groth16 toy m=21": (("toy", "groth16", 21, False), {}),
    "rinocchio zk toy m=21": (("toy", "rinocchio", 21, True), {}),
    "groth16 C2 m=8 prover_lin_io=1": (("C2", "groth16", 8, False, False), {"prover_lin_io": 1}),
    "groth16 C2 m=8 prover_lin_io=0": (("C2", "groth16", 8, False, False), {"prover_lin_io": 0}),
    "groth16 C2 m=3": (("C2", "groth16", 3, False, False), {}),
    "groth16 toy m=21 seeded device key msm_host_tile=8": (("toy", "groth16", 21, False), {"msm_host_tile": 8}),
}
CALLS = [(label, B) for label in KEYS for B in ((0, 3) if "seeded" in label else (0, 1, 3))]  # B = 0: the single prover
BYTES = {"toy m=21": ("toy", "groth16", 21, False), "C2 m=8": ("C2", "groth16", 8, False, False)}  # label -> batch_case arguments


def call_id(label, B):
    return "%s, %s" % (label, "single" if B == 0 else "batch of %d" % B)


def record_launches(label, B):
    from ringsnark_amd import _lib
    args, knobs = KEYS[label]
    c = batch_case(*args)
    dev, dcs, scheme = c["dev"], c["dcs"], args[1]
    pk = c["pk"] if "seeded" in label else c["wide"]
    if B == 0:
        fn = lambda: prove(dev, scheme, dcs, pk, c["asgs"][0], (None, None, None) if c["ds"] is None else c["ds"][0])
    else:
        fn = lambda: prove_batch(dev, scheme, dcs, pk, c["asgs"][:B], stack_d(dev, c["ds"], B))
    with _lib.tuning(**knobs):
        fn()
        return launches(dev, fn)


def record_bytes(label):
    c = batch_case(*BYTES[label])  # the bytes depend on the system and the context only, not on the key's scheme
    return {scheme: [c["dev"].prove_batch_bytes(c["dcs"], scheme, B) for B in (1, 2, 3, 8)] for scheme in ("groth16", "rinocchio")}


def record():
    return {"launches": {call_id(label, B): record_launches(label, B) for label, B in CALLS},
            "prove_batch_bytes, batch 1 2 3 8": {label: record_bytes(label) for label in BYTES}}


@pytest.fixture(scope="module")
def golden():
    return json.load(open(FIXTURE))


@pytest.mark.gpu
@pytest.mark.parametrize("label,B", CALLS, ids=[call_id(*c) for c in CALLS])
def test_prover_launches_what_it_launched_before_the_merge(golden, label, B):
    exp = golden["launches"][call_id(label, B)]
    assert exp and record_launches(label, B) == exp


@pytest.mark.gpu
@pytest.mark.parametrize("label", BYTES)
def test_batch_workspace_bytes_are_what_they_were_before_the_merge(golden, label):
    exp = golden["prove_batch_bytes, batch 1 2 3 8"][label]
    assert all(len(v) == 4 and min(v) > 0 for v in exp.values()) and record_bytes(label) == exp
