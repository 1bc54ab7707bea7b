"""The multiply-accumulate kernels of the inner product on sign-aligned worst-case sums (builders and their derivation:
tests/helpers.py; the conditions on the inputs: tests/test_aligned_inputs.py).

Every FP64 kernel holds lazily reduced balanced integers in doubles and brings its accumulators back only every
`acc_period` terms (csrc/msm.hip).  Random data never comes near the bound that period protects, and with few terms a chunk
holds one term, so the branch does not even run.  Here every product of a (limb, component, prime) slab is a chosen integer
of about 0.30 Q_j with one sign, T = aligned_T(Q) terms of them pass 2^53, and one chunk takes all the terms of a tile
(mac_chunk_units = 1, untiled key): an accumulator that is not reduced in time leaves the exactly representable integers
and the result is wrong.  The expected value is the closed form sum_t target_t mod Q_j in Python integers; the smaller
contexts are checked against the CPU oracle as well.  All comparisons are integer equality.  Needs a real MI355X."""
import numpy as np
import pytest

from ringsnark_amd import _lib
from tests import helpers as H

pytestmark = pytest.mark.gpu

D = H.ALIGNED_D
_DEV, _IN, _ORACLE = {}, {}, {}

# the knob settings every case runs under: one chunk per tile (the accumulators take every term of the tile: the periodic
# reduction), the default chunks (summed by reduce_kernel), term tiles of 1 MiB of plaintext rows (a launch per tile that
# starts from the canonical partial sums of the one before), and such tiles with one chunk
RUNS = (("one chunk", dict(mac_chunk_units=1)), ("default chunks", {}), ("tiles", dict(msm_c_mib=1)),
        ("tiles, one chunk", dict(msm_c_mib=1, mac_chunk_units=1)))


def dev_for(name):
    from ringsnark_amd.device import Device
    if name not in _DEV:
        _DEV[name] = Device(H.worst_case_params(name))
    return _DEV[name]


def host(t):
    from ringsnark_amd.device import to_host
    return to_host(t)


def expand(dev, a, T):
    """[D]... on the host -> [T]... on the device, term t = a[t % D]"""
    import torch
    idx = torch.arange(T, device=dev.device) % a.shape[0]
    return dev.put(np.ascontiguousarray(a))[idx].contiguous()


def inputs(name, variant, key=0):
    """Device tensors of H.aligned_case, its closed form, and the conditions on the inputs checked on what is uploaded."""
    if (name, variant, key) not in _IN:
        dev = dev_for(name)
        ctx, rings, encs, targets, T, kinds = H.aligned_case(name, variant, key)
        reached = H.check_aligned_inputs(ctx, targets, T)
        print("%s/%s key %d: T = %d, key %.1f MiB, never-reduced sums reach %.3f x 2^53 or more" % (name, variant, key, T, T * ctx.enc_words * 8 / 2.0**20, reached))
        _IN[(name, variant, key)] = dict(ctx=ctx, T=T, key=expand(dev, encs, T), rows=expand(dev, rings, T),
                                         kinds=None if kinds is None else np.ascontiguousarray(kinds[np.arange(T) % D]),
                                         exp=H.closed_form(ctx, targets, T))
    return _IN[(name, variant, key)]


def oracle_value(name, key):
    if (name, key) not in _ORACLE:
        ctx, rings, encs, targets, T, kinds = H.aligned_case(name, "poly", key)
        _ORACLE[(name, key)] = ctx.inner_product(encs, np.ascontiguousarray(rings[np.arange(T) % D]), threads=0, window=D)[0]
    return _ORACLE[(name, key)]


def run_msm(dev, keys, vecs, n_groups, knobs):
    """-> (result [n_keys][n_groups] on the host, names of the kernels that ran)"""
    with _lib.tuning(**knobs):
        dev.set_profiling(True)
        try:
            dev.profile_read()
            out, _ = dev.msm(keys, vecs, n_groups)
            got = host(out)
            names = {k["name"] for k in dev.profile_read()}
        finally:
            dev.set_profiling(False)
    return got, names


def check_case(name, variant, n_groups, n_keys, knobs, kernels, oracle):
    """The aligned terms of (name, variant): every group multiplies the same rows, every key has targets of its own.  Runs
    under `knobs` plus each of RUNS; `kernels`: profile names that must have run (all of them) -- the other multiply-accumulate
    kernels must not."""
    dev = dev_for(name)
    ins = [inputs(name, variant, k) for k in range(n_keys)]
    first = ins[0]
    vecs = [(first["rows"], first["kinds"], g) + ((True,) if variant == "const" else ()) for g in range(n_groups)]
    for label, run in RUNS:
        got, names = run_msm(dev, [x["key"] for x in ins], vecs, n_groups, {**knobs, **run})
        macs = {k for k in names if k.startswith("mac_kernel")}
        assert macs == {k for k in kernels if k.startswith("mac_kernel")} and set(kernels) <= names, (label, names)
        for k in range(n_keys):
            for g in range(n_groups):
                bad = got[k, g] != ins[k]["exp"]
                assert not bad.any(), "%s, %s: key %d group %d: %d of %d words differ from the closed form (T = %d), first at %s" % (
                    name, label, k, g, int(bad.sum()), bad.size, first["T"], tuple(np.argwhere(bad)[0]))
    if oracle:
        for k in range(n_keys):
            assert (ins[k]["exp"] == oracle_value(name, k)).all(), (name, k)


WIDE, PLAIN = "plain_center_wide_kernel", "plain_center_kernel"
CASES = [
    # context, variant, groups, keys, knobs, kernels that must run, also against the oracle
    # 1: the generic kernel, PAIRS = 4, its three instantiations
    ("toy49", "poly", 1, 1, {}, ("mac_kernel",), True),
    ("toy49", "poly", 2, 1, {}, ("mac_kernel",), True),
    ("toy49", "poly", 1, 2, {}, ("mac_kernel",), True),
    ("toy49", "one", 2, 1, {}, ("mac_kernel",), False),
    ("toy49", "const", 1, 2, {}, ("mac_kernel",), False),
    # 2: 2048 points, the streaming kernel and the generic one
    ("n2048", "poly", 1, 1, {}, ("mac_kernel_v2",), True),
    ("n2048", "poly", 1, 1, dict(mac_variant=1), ("mac_kernel",), True),
    ("n2048", "one", 1, 1, {}, ("mac_kernel_v2",), False),
    ("n2048", "const", 1, 1, {}, ("mac_kernel_v2",), False),
    # 3: 8192 points: half spectrum on paired and on natural rows, the streaming kernel, two keys on paired and natural rows
    ("n8192", "poly", 1, 1, {}, ("mac_kernel_v3", WIDE), True),
    ("n8192", "poly", 2, 1, dict(plain_variant=0), ("mac_kernel_v3", PLAIN), True),
    ("n8192", "poly", 1, 1, dict(mac_variant=3), ("mac_kernel_v2", WIDE), True),
    ("n8192", "poly", 1, 2, {}, ("mac_kernel_v4<13, true>", WIDE), True),
    ("n8192", "poly", 2, 2, dict(plain_variant=0), ("mac_kernel_v4<13, false>", PLAIN), True),
    ("n8192", "one", 1, 1, {}, ("mac_kernel_v3", WIDE), False),
    ("n8192", "const", 1, 1, {}, ("mac_kernel_v3", WIDE), False),
    ("n8192", "one", 1, 2, {}, ("mac_kernel_v4<13, true>", WIDE), False),
    ("n8192", "const", 1, 2, dict(plain_variant=0), ("mac_kernel_v4<13, false>", PLAIN), False),
    # 4: 16384 points: quarter spectrum, two keys, the generic kernel with PAIRS = 8
    ("n16384", "poly", 1, 1, {}, ("mac_kernel_v3<false, 14>",), False),
    ("n16384", "poly", 1, 2, {}, ("mac_kernel_v4<14, false>",), False),
    ("n16384", "poly", 1, 1, dict(mac_variant=1), ("mac_kernel",), False),
    # 5: a 44-bit prime of the headline's size: the accumulator period is 319 terms, T five of them
    ("n8192q44", "poly", 1, 1, {}, ("mac_kernel_v3", WIDE), False),
    ("n8192q44", "poly", 1, 2, {}, ("mac_kernel_v4<13, true>", WIDE), False),
    # 6: hybrid context: 54-bit ring prime on the integer arithmetic, FP64 multiply-accumulate of the 48 / 49-bit data primes
    ("hybrid8192", "poly", 1, 1, {}, ("mac_kernel_v3", PLAIN), False),
    ("hybrid8192", "poly", 2, 2, {}, ("mac_kernel_v4<13, false>", PLAIN), False),
    # 7: the rows of 1-4 and 6 on primes just below 2^50, the largest the FP64 arithmetic accepts: the accumulator period is
    # 4 terms, the shortest there is, and four products of up to 0.875 p each leave reduce() no room beyond 2^52 = 4 p
    ("toy50", "poly", 1, 1, {}, ("mac_kernel",), True),
    ("toy50", "poly", 2, 1, {}, ("mac_kernel",), True),
    ("toy50", "poly", 1, 2, {}, ("mac_kernel",), True),
    ("toy50", "one", 2, 1, {}, ("mac_kernel",), False),
    ("toy50", "const", 1, 2, {}, ("mac_kernel",), False),
    ("n2048q50", "poly", 1, 1, {}, ("mac_kernel_v2",), True),
    ("n2048q50", "poly", 1, 1, dict(mac_variant=1), ("mac_kernel",), True),
    ("n2048q50", "one", 1, 1, {}, ("mac_kernel_v2",), False),
    ("n2048q50", "const", 1, 1, {}, ("mac_kernel_v2",), False),
    ("n8192q50", "poly", 1, 1, {}, ("mac_kernel_v3", WIDE), True),
    ("n8192q50", "poly", 2, 1, dict(plain_variant=0), ("mac_kernel_v3", PLAIN), True),
    ("n8192q50", "poly", 1, 1, dict(mac_variant=3), ("mac_kernel_v2", WIDE), True),
    ("n8192q50", "poly", 1, 2, {}, ("mac_kernel_v4<13, true>", WIDE), True),
    ("n8192q50", "poly", 2, 2, dict(plain_variant=0), ("mac_kernel_v4<13, false>", PLAIN), True),
    ("n8192q50", "one", 1, 1, {}, ("mac_kernel_v3", WIDE), False),
    ("n8192q50", "const", 1, 1, {}, ("mac_kernel_v3", WIDE), False),
    ("n8192q50", "one", 1, 2, {}, ("mac_kernel_v4<13, true>", WIDE), False),
    ("n8192q50", "const", 1, 2, dict(plain_variant=0), ("mac_kernel_v4<13, false>", PLAIN), False),
    ("n16384q50", "poly", 1, 1, {}, ("mac_kernel_v3<false, 14>",), False),
    ("n16384q50", "poly", 1, 2, {}, ("mac_kernel_v4<14, false>",), False),
    ("n16384q50", "poly", 1, 1, dict(mac_variant=1), ("mac_kernel",), False),
    ("hybrid8192q50", "poly", 1, 1, {}, ("mac_kernel_v3", PLAIN), False),
    ("hybrid8192q50", "poly", 2, 2, {}, ("mac_kernel_v4<13, false>", PLAIN), False),
]


@pytest.mark.parametrize("name,variant,n_groups,n_keys,knobs,kernels,oracle", CASES,
                         ids=["%s-%s-g%dk%d-%s" % (c[0], c[1], c[2], c[3], "-".join("%s%d" % kv for kv in c[4].items()) or "default") for c in CASES])
def test_aligned_sums_equal_the_closed_form(name, variant, n_groups, n_keys, knobs, kernels, oracle):
    check_case(name, variant, n_groups, n_keys, knobs, kernels, oracle)


EXTREME_KERNEL = {"n8192": "mac_kernel_v3", "hybrid8192": "mac_kernel_v3", "n16384full": "mac_kernel_v3<false, 14>",
                  "n8192q50": "mac_kernel_v3"}


@pytest.mark.parametrize("name", sorted(H.EXTREME_CASES))
def test_plaintext_rows_at_the_ends_of_the_balanced_range(name):
    """Every plaintext coefficient at +-(q - 1) / 2 (tests/helpers.py: extreme_rows; all plus, all minus, alternating, random).
    FP64 contexts: a group of MAX_GROUP_VECS = 4 such vectors with the same rows, so every coefficient of the summed row is
    +-2 (q - 1), the bound b0 the reduction masks of the forward transform are built for.  Hybrid context: one vector per
    group, rows at +-(q - 1) / 2 of the 54-bit prime -- doubles just under 2^53.  A handful of terms against a random key and
    the oracle (enc_add across the group's vectors), then T = aligned_T terms against the key aligned to the summed row."""
    dev = dev_for(name)
    ctx, rings, n_vecs, encs, targets, T = H.extreme_case(name)
    kernel = EXTREME_KERNEL[name]
    # a handful of terms, random key, two groups, against the oracle
    t = 5
    key = ctx.random_enc(77, t)
    drows = dev.put(np.ascontiguousarray(rings[:t]))
    vecs = [(drows, None, g) for g in range(2) for _ in range(n_vecs)]
    one = ctx.inner_product(key, np.ascontiguousarray(rings[:t]), threads=0)[0]
    exp = one
    for _ in range(n_vecs - 1):
        exp = ctx.enc_add(exp, one)
    for knobs in ({}, dict(mac_chunk_units=1)):
        got, names = run_msm(dev, [dev.put(key)], vecs, 2, knobs)
        assert {k for k in names if k.startswith("mac_kernel")} == {kernel}, names
        assert (got[0, 0] == exp).all() and (got[0, 1] == exp).all(), (name, knobs)
    # aligned key for the summed row
    reached = H.check_aligned_inputs(ctx, targets, T)
    print("%s/extreme: T = %d, key %.1f MiB, never-reduced sums reach %.3f x 2^53 or more" % (name, T, T * ctx.enc_words * 8 / 2.0**20, reached))
    exp = H.closed_form(ctx, targets, T)
    dkey, drows = expand(dev, encs, T), expand(dev, rings, T)
    for label, run in RUNS:
        got, names = run_msm(dev, [dkey], [(drows, None, 0)] * n_vecs, 1, run)
        assert {k for k in names if k.startswith("mac_kernel")} == {kernel}, (label, names)
        bad = got[0, 0] != exp
        assert not bad.any(), "%s, %s: %d of %d words differ from the closed form (T = %d)" % (name, label, int(bad.sum()), bad.size, T)
