"""Device context: the Python host side above the C ABI (include/ringsnark_amd.h).

PyTorch is used for what it is good at here -- device memory, streams, torch.distributed -- and
nothing else: every arithmetic operation goes through librs_hip.so.  Residues live in int64 CUDA
tensors (bit-identical to the uint64 boundary layout; all values are < 2^50).
"""
import collections
import ctypes as C

import numpy as np
import torch

from . import _lib
from .params import RingParams
from .r1cs import R1CS, SOLVE_BLOCKED, HintReport, HintSolveInfo, InvReport, R1csCheck, SolveInfo, given_mask, plaintext_check_layout


def to_device(a: np.ndarray, device) -> torch.Tensor:
    a = np.ascontiguousarray(a, dtype=np.uint64)
    return torch.from_numpy(a.view(np.int64)).to(device)


def to_host(t: torch.Tensor) -> np.ndarray:
    return t.detach().cpu().contiguous().numpy().view(np.uint64)


def _ptr(t):
    if t is None:
        return None
    assert t.is_cuda and t.is_contiguous() and t.dtype == torch.int64, (t.device, t.dtype, t.is_contiguous())
    return C.c_void_p(t.data_ptr())


class HostWords:
    """Page-locked host buffer of uint64 words (rs_host_alloc); `array` is a numpy view of it."""

    def __init__(self, dev, words):
        self.dev, self.words = dev, int(words)
        p = C.c_void_p()
        _lib.check(dev.lib.rs_host_alloc(dev.h, self.words * 8, C.byref(p)))
        self.ptr = p.value
        self.array = np.ctypeslib.as_array((C.c_uint64 * self.words).from_address(self.ptr))

    def fill_from(self, tensor, offset_words=0):
        """device tensor (int64) -> this buffer at offset_words (rs_download)."""
        t = tensor.contiguous()
        assert offset_words + t.numel() <= self.words
        _lib.check(self.dev.lib.rs_download(self.dev.h, C.c_void_p(self.ptr + 8 * offset_words), C.c_void_p(t.data_ptr()), t.numel() * 8, self.dev.stream()))
        self.dev.sync()

    def __del__(self):
        if getattr(self, "ptr", None) and self.dev.lib is not None and getattr(self.dev, "h", None):
            self.array = None
            self.dev.lib.rs_host_free(self.dev.h, C.c_void_p(self.ptr))
            self.ptr = None


class DeviceR1CS:
    def __init__(self, dev, cs: R1CS):
        self.dev, self.cs = dev, cs
        self.m, self.n_vars, self.n_inputs = cs.m, cs.n_vars, cs.n_inputs
        rp = (_lib.u32p * 3)()
        col = (_lib.u32p * 3)()
        cf = (_lib.u64p * 3)()
        nnz = (C.c_size_t * 3)()
        keep = []
        for k, name in enumerate("abc"):
            r, c, f = cs.mats[name]
            r = np.ascontiguousarray(r, dtype=np.uint32)
            c = np.ascontiguousarray(c, dtype=np.uint32)
            f = np.ascontiguousarray(f, dtype=np.uint64)
            assert f.shape == (dev.L, c.shape[0])
            keep += [r, c, f]
            rp[k] = r.ctypes.data_as(_lib.u32p)
            col[k] = c.ctypes.data_as(_lib.u32p)
            cf[k] = f.ctypes.data_as(_lib.u64p)
            nnz[k] = c.shape[0]
        h = C.c_void_p()
        if cs.poly_table is None:
            _lib.check(dev.lib.rs_r1cs_create(dev.h, cs.m, cs.n_vars, cs.n_inputs, rp, col, cf, nnz, C.byref(h)))
        else:  # coefficients that are general ring elements (relations/variable.tcc:246-254)
            i32p = C.POINTER(C.c_int32)
            pidx = (i32p * 3)()
            for k, name in enumerate("abc"):
                pi = np.ascontiguousarray(cs.poly_idx[name], dtype=np.int32)
                assert pi.shape[0] == nnz[k]
                keep.append(pi)
                pidx[k] = pi.ctypes.data_as(i32p)
            tab = np.ascontiguousarray(cs.poly_table, dtype=np.uint64)
            assert tab.shape[1:] == (dev.L, dev.N)
            _lib.check(dev.lib.rs_r1cs_create_poly(dev.h, cs.m, cs.n_vars, cs.n_inputs, rp, col, cf, nnz, pidx,
                                                   tab.ctypes.data_as(_lib.u64p), tab.shape[0], C.byref(h)))
        self.h = h

    def __del__(self):
        if getattr(self, "h", None) and self.dev.lib is not None:
            self.dev.lib.rs_r1cs_destroy(self.h)
            self.h = None


SOLVE_MODES = {"auto": _lib.RS_SOLVE_AUTO, "levels": _lib.RS_SOLVE_LEVELS, "walk": _lib.RS_SOLVE_WALK}
SolveStats = collections.namedtuple("SolveStats", "level_launches walk_launches")


class SolvePlan:
    """A solve plan on the device (rs_r1cs_solve_plan): the schedule that completes an assignment of `dcs` from the given
    wires.  .info is a SolveInfo; close() (or garbage collection) frees it.  Keeps `dcs` alive: the plan reads its matrices."""

    def __init__(self, dev, dcs, given):
        self.dev, self.dcs = dev, dcs
        mask = given_mask(dcs.cs, given)
        h, info = C.c_void_p(), _lib.SolveInfo()
        _lib.check(dev.lib.rs_r1cs_solve_plan_create(dev.h, dcs.h, mask.ctypes.data_as(_lib.u8p), C.byref(h), C.byref(info)))
        self.h = h
        self.info = SolveInfo(*[int(getattr(info, k)) for k, _ in _lib.SolveInfo._fields_])

    def steps(self):
        """([(constraint, variable)] in the order they run, level_ptr [n_levels + 1])"""
        n = self.info.n_solved
        rows, wires = np.zeros(max(n, 1), dtype=np.uint32), np.zeros(max(n, 1), dtype=np.uint32)
        lp = np.zeros(self.info.n_levels + 1, dtype=np.uint64)
        _lib.check(self.dev.lib.rs_r1cs_solve_plan_steps(self.h, rows.ctypes.data_as(_lib.u32p), wires.ctypes.data_as(_lib.u32p),
                                                         lp.ctypes.data_as(_lib.u64p)))
        return [(int(r), int(w)) for r, w in zip(rows[:n], wires[:n])], [int(x) for x in lp]

    def close(self):
        if getattr(self, "h", None) and self.dev.lib is not None:
            self.dev.lib.rs_r1cs_solve_plan_destroy(self.h)
        self.h = None

    __del__ = close


HintSolveStats = collections.namedtuple("HintSolveStats", "level_launches walk_launches hint_launches")


class HintPlan:
    """A solve plan with hints on the device (rs_r1cs_hint_plan of ringsnark_amd/solve_hints.h): the schedule that completes an
    assignment of `dcs` from the given wires and the declared hints (ringsnark_amd.r1cs.Hint).  .info is a HintSolveInfo;
    close() (or garbage collection) frees it.  Keeps `dcs` alive: the plan reads its matrices."""

    def __init__(self, dev, dcs, given, hints):
        self.dev, self.dcs, self.hints = dev, dcs, list(hints)
        mask = given_mask(dcs.cs, given)
        arr = (_lib.SolveHint * max(len(self.hints), 1))(*[_lib.SolveHint(h.kind, h.src, h.num, h.dst, h.nbits, h.dst_stride)
                                                          for h in self.hints])
        h, info = C.c_void_p(), _lib.HintInfo()
        _lib.check(dev.lib.rs_r1cs_hint_plan_create(dev.h, dcs.h, mask.ctypes.data_as(_lib.u8p), arr if self.hints else None,
                                                    len(self.hints), C.byref(h), C.byref(info)))
        self.h = h
        self.info = HintSolveInfo(*[int(getattr(info.solve, k)) for k, _ in _lib.SolveInfo._fields_], int(info.n_steps),
                                  int(info.n_hints_run), int(info.n_hints_blocked), int(info.first_blocked_hint))

    def steps(self):
        """([(kind, index, wire)] in the order they run -- kind 0: constraint and target, kind 1: hint and its first target --,
        level_ptr [n_levels + 1])"""
        n = self.info.n_steps
        kind = np.zeros(max(n, 1), dtype=np.uint8)
        index, wire = np.zeros(max(n, 1), dtype=np.uint32), np.zeros(max(n, 1), dtype=np.uint32)
        lp = np.zeros(self.info.n_levels + 1, dtype=np.uint64)
        _lib.check(self.dev.lib.rs_r1cs_hint_plan_steps(self.h, kind.ctypes.data_as(_lib.u8p), index.ctypes.data_as(_lib.u32p),
                                                        wire.ctypes.data_as(_lib.u32p), lp.ctypes.data_as(_lib.u64p)))
        return [(int(k), int(i), int(w)) for k, i, w in zip(kind[:n], index[:n], wire[:n])], [int(x) for x in lp]

    def close(self):
        if getattr(self, "h", None) and self.dev.lib is not None:
            self.dev.lib.rs_r1cs_hint_plan_destroy(self.h)
        self.h = None

    __del__ = close


IO_EVAL_TILE = 64  # rows per tile of rs_io_eval_at (csrc/verify.hip IO_TILE): its workspace is 2 * ceil(m / 64) ring elements


class VerifyResult(collections.namedtuple("VerifyResult", "accepted failed n_bad first_check first_limb first_slot lhs rhs")):
    """rs_verify_report (ringsnark_amd/verify.h), field for field; n_bad is a tuple of six counts."""
    __slots__ = ()

    def __bool__(self):
        return bool(self.accepted)


class BatchVerdict(collections.namedtuple("BatchVerdict", "result noise_spent budget_min")):
    """One member of a batched verification (ringsnark_amd/verify_batch.h): result is the member's VerifyResult, or None
    when its noise budget is spent (noise_spent; the single verifier raises RS_ERR_NOISE there); budget_min is the smallest
    noise budget over its non-EMPTY ciphertexts.  True when the proof is accepted."""
    __slots__ = ()

    def __bool__(self):
        return self.result is not None and bool(self.result.accepted)


class BitsResult(collections.namedtuple("BitsResult", "n_bad first_elem first_limb first_slot word value")):
    """rs_bits_report (ringsnark_amd/bits.h), field for field; true when no position is bad."""
    __slots__ = ()

    def __bool__(self):
        return self.n_bad == 0


class DeviceVK:
    """A verification key on the device (rs_groth16_vk / rs_rinocchio_vk): the public columns of the instance map at s,
    Z(s), the trapdoor elements and the secret key.  close() (or garbage collection) zeroes and frees it."""

    def __init__(self, dev, scheme, handle, n_inputs):
        self.dev, self.scheme, self.h, self.n_inputs = dev, scheme, handle, n_inputs

    def close(self):
        if getattr(self, "h", None) and self.dev.lib is not None:
            (self.dev.lib.rs_groth16_vk_destroy if self.scheme == "groth16" else self.dev.lib.rs_rinocchio_vk_destroy)(self.h)
        self.h = None

    __del__ = close


class Device:
    """rs_ctx wrapper.  Mirrors RingElem::set_context + EncodingElem::set_context
    (seal/seal_ring.hpp:52-58, 266-320): one object per (process, GPU)."""

    def __init__(self, prm: RingParams, device_index: int = 0):
        self.lib = _lib.load()  # raises if librs_hip.so is missing -- no fallback
        if not torch.cuda.is_available():
            raise RuntimeError("ringsnark_amd needs a HIP device (torch.cuda.is_available() is False)")
        self.prm = prm
        self.N, self.L, self.N_enc, self.K = prm.N, prm.L, prm.N_enc, prm.K
        self.device = torch.device("cuda", device_index)
        torch.cuda.set_device(self.device)
        q = (C.c_uint64 * self.L)(*prm.q)
        Q = (C.c_uint64 * self.K)(*prm.Q)
        h = C.c_void_p()
        _lib.check(self.lib.rs_ctx_create(device_index, self.N, self.L, q, self.N_enc, self.K, Q, C.byref(h)))
        self.h = h
        self.ring_words, self.enc_words = prm.ring_words, prm.enc_words

    def __del__(self):
        if getattr(self, "h", None) and self.lib is not None:
            self.lib.rs_ctx_destroy(self.h)
            self.h = None

    # ---- helpers
    def stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def ring_empty(self, *lead):
        return torch.empty(tuple(lead) + (self.L, self.N), dtype=torch.int64, device=self.device)

    def enc_empty(self, *lead):
        return torch.empty(tuple(lead) + (self.L, 2, self.K, self.N_enc), dtype=torch.int64, device=self.device)

    def put(self, a):
        return to_device(a, self.device)

    def sync(self):
        _lib.check(self.lib.rs_sync(self.h, self.stream()))

    @staticmethod
    def _count(t, words):
        assert t.numel() % words == 0
        return t.numel() // words

    # ---- a4
    def ntt(self, data, modset, index, inverse=False):
        """In-place batched negacyclic NTT over [batch][N_enc]."""
        batch = self._count(data, self.N_enc)
        fn = self.lib.rs_ntt_inverse if inverse else self.lib.rs_ntt_forward
        _lib.check(fn(self.h, modset, index, _ptr(data), batch, self.stream()))
        return data

    # ---- a1-a3
    def _bin(self, fn, a, b):
        a, b = a.contiguous(), b.contiguous()
        out = torch.empty_like(a)
        _lib.check(fn(self.h, _ptr(out), _ptr(a), _ptr(b), self._count(a, self.ring_words), self.stream()))
        return out

    def ring_add(self, a, b):
        return self._bin(self.lib.rs_ring_add, a, b)

    def ring_sub(self, a, b):
        return self._bin(self.lib.rs_ring_sub, a, b)

    def ring_mul(self, a, b):
        return self._bin(self.lib.rs_ring_mul, a, b)

    def ring_neg(self, a):
        out = torch.empty_like(a)
        _lib.check(self.lib.rs_ring_neg(self.h, _ptr(out), _ptr(a), self._count(a, self.ring_words), self.stream()))
        return out

    def ring_add_scalar(self, a, s):
        a = a.contiguous()
        out = torch.empty_like(a)
        _lib.check(self.lib.rs_ring_add_scalar(self.h, _ptr(out), _ptr(a), s, self._count(a, self.ring_words), self.stream()))
        return out

    def ring_mul_scalar(self, a, s):
        a = a.contiguous()
        out = torch.empty_like(a)
        _lib.check(self.lib.rs_ring_mul_scalar(self.h, _ptr(out), _ptr(a), s, self._count(a, self.ring_words), self.stream()))
        return out

    def ring_inv(self, a):
        """Raises RsError(RS_ERR_NOT_INVERTIBLE, "element is not invertible in ring")."""
        out = torch.empty_like(a)
        _lib.check(self.lib.rs_ring_inv(self.h, _ptr(out), _ptr(a), self._count(a, self.ring_words), self.stream()))
        return out

    def ring_is_zero(self, a):
        count = self._count(a, self.ring_words)
        flags = (C.c_uint8 * count)()
        _lib.check(self.lib.rs_ring_is_zero(self.h, _ptr(a), count, flags, self.stream()))
        return [bool(f) for f in flags]

    # ---- a5-a8
    def batch_encode(self, rings):
        count = self._count(rings, self.ring_words)
        out = torch.empty((count, self.L, self.N_enc), dtype=torch.int64, device=self.device)
        _lib.check(self.lib.rs_batch_encode(self.h, _ptr(rings), _ptr(out), count, self.stream()))
        return out

    def enc_mul_ring(self, enc, ring):
        enc = enc.clone()
        _lib.check(self.lib.rs_enc_mul_ring(self.h, _ptr(enc), _ptr(ring), self._count(enc, self.enc_words), self.stream()))
        return enc

    def enc_add(self, a, b):
        out = torch.empty_like(a)
        _lib.check(self.lib.rs_enc_add(self.h, _ptr(out), _ptr(a), _ptr(b), self._count(a, self.enc_words), self.stream()))
        return out

    def enc_reduce(self, enc):
        """In-place x mod Q_j on integer sums of encoding elements (multi-GPU all-reduce epilogue)."""
        _lib.check(self.lib.rs_enc_reduce(self.h, _ptr(enc), self._count(enc, self.enc_words), self.stream()))
        return enc

    # ---- 8(f) f2: instance map with evaluation
    def instance_map_eval(self, dcs, s):
        """r1cs_to_qrp_instance_map_with_evaluation (r1cs_to_qrp.tcc:76-116): returns At, Bt, Ct
        [n_vars+1][L][N], Ht [m+1][L][N], Zt [L][N] for the point s [L][N]."""
        n1 = dcs.cs.n_vars + 1
        At, Bt, Ct = self.ring_empty(n1), self.ring_empty(n1), self.ring_empty(n1)
        Ht, Zt = self.ring_empty(dcs.cs.m + 1), self.ring_empty()
        _lib.check(self.lib.rs_instance_map_eval(self.h, dcs.h, _ptr(s), _ptr(At), _ptr(Bt), _ptr(Ct), _ptr(Ht), _ptr(Zt),
                                                 self.stream()))
        return At, Bt, Ct, Ht, Zt

    # ---- verifiers (ringsnark_amd/verify.h)
    def io_eval_at(self, dcs, s):
        """rs_io_eval_at: (Aio, Bio, Cio [n_inputs+1][L][N], Zt [L][N]) -- rows 0..n_inputs of instance_map_eval's At, Bt, Ct
        and its Zt, bit for bit, without the [m][L][N] Lagrange values or the [n_vars+1][L][N] outputs."""
        n1 = dcs.n_inputs + 1
        A, B, Cc, Zt = self.ring_empty(n1), self.ring_empty(n1), self.ring_empty(n1), self.ring_empty()
        _lib.check(self.lib.rs_io_eval_at(self.h, dcs.h, _ptr(s), _ptr(A), _ptr(B), _ptr(Cc), _ptr(Zt), self.stream()))
        return A, B, Cc, Zt

    def _vk_part(self, v):
        return v if isinstance(v, torch.Tensor) else self.put(v)

    def groth16_vk(self, dcs, vk):
        """vk: dict s, alpha, beta, gamma, delta ([L][N]) and sk ([K][N_enc], NTT form), numpy or device tensors -- what
        tests/snark_ref.py's generator returns.  RsError(RS_ERR_NOT_INVERTIBLE) unless gamma is a unit (groth16.tcc:162)."""
        t = [self._vk_part(vk[k]) for k in ("s", "alpha", "beta", "gamma", "delta", "sk")]
        self.sync()
        h = C.c_void_p()
        _lib.check(self.lib.rs_groth16_vk_create(self.h, dcs.h, *[_ptr(x) for x in t], C.byref(h)))
        return DeviceVK(self, "groth16", h, dcs.n_inputs)

    def rinocchio_vk(self, dcs, vk):
        """vk: dict s, alpha, beta, r_v, r_w, r_y and sk."""
        t = [self._vk_part(vk[k]) for k in ("s", "alpha", "beta", "r_v", "r_w", "r_y", "sk")]
        self.sync()
        h = C.c_void_p()
        _lib.check(self.lib.rs_rinocchio_vk_create(self.h, dcs.h, *[_ptr(x) for x in t], C.byref(h)))
        return DeviceVK(self, "rinocchio", h, dcs.n_inputs)

    def _verify(self, fn, vk, scheme, n_elems, primary, proof, empty, level=None):
        assert vk.scheme == scheme and vk.h, "not a live %s verification key" % scheme
        assert self._count(proof, self.level_words(level)) == n_elems
        assert vk.n_inputs == 0 or self._count(primary, self.ring_words) == vk.n_inputs
        em = None if empty is None else (C.c_int * n_elems)(*[int(e) for e in empty])
        rep = _lib.VerifyReport()
        lvl = () if level is None else (int(level),)
        _lib.check(fn(self.h, vk.h, *lvl, _ptr(primary) if vk.n_inputs else None, _ptr(proof), em, C.byref(rep), self.stream()))
        return VerifyResult(bool(rep.accepted), int(rep.failed), tuple(int(x) for x in rep.n_bad), int(rep.first_check),
                            int(rep.first_limb), int(rep.first_slot), int(rep.lhs), int(rep.rhs))

    def groth16_verify(self, vk, primary, proof, empty=None, level=None):
        """groth16::verifier (groth16.tcc:117-170): primary [n_inputs][L][N], proof [3] encoding elements, empty: the flags
        the prover returned.  A VerifyResult (truthy when accepted); RsError(RS_ERR_NOISE) for a proof past its noise budget.
        level: the proof was switched to that many primes (enc_mod_switch; rs_groth16_verify_level)."""
        fn = self.lib.rs_groth16_verify if level is None else self.lib.rs_groth16_verify_level
        return self._verify(fn, vk, "groth16", 3, primary, proof, empty, level)

    def rinocchio_verify(self, vk, primary, proof, empty=None, level=None):
        """rinocchio::verifier (rinocchio.tcc:192-295): proof [9]; failed bit c = check c of verify.h (V', W', Y', H', L_beta, P).
        level: as in groth16_verify (rs_rinocchio_verify_level)."""
        fn = self.lib.rs_rinocchio_verify if level is None else self.lib.rs_rinocchio_verify_level
        return self._verify(fn, vk, "rinocchio", 9, primary, proof, empty, level)

    # ---- a batch of proofs against one key (ringsnark_amd/verify_batch.h)
    def _stacked(self, items, words, what):
        """a list of tensors, or one stacked tensor [B][...], as one contiguous tensor and its count B"""
        t = items if isinstance(items, torch.Tensor) else torch.stack([x.contiguous() for x in items])
        t = t.contiguous()
        assert t.numel() % words == 0, "%s: not a whole number of members" % what
        return t, t.numel() // words

    def _verify_batch(self, fn, vk, scheme, n_elems, primaries, proofs, empties, level):
        assert vk.scheme == scheme and vk.h, "not a live %s verification key" % scheme
        K_lvl = self.K if level is None else int(level)
        proofs, B = self._stacked(proofs, n_elems * self.level_words(K_lvl), "proofs")
        if vk.n_inputs:
            primaries, Bp = self._stacked(primaries, vk.n_inputs * self.ring_words, "primary inputs")
            assert Bp == B, "as many primary inputs as proofs"
        assert empties is None or len(empties) == B
        out = []
        for b0 in range(0, B, _lib.VERIFY_BATCH_MAX):
            nb = min(_lib.VERIFY_BATCH_MAX, B - b0)
            em = None if empties is None else (C.c_int * (nb * n_elems))(*[int(e) for row in empties[b0:b0 + nb] for e in row])
            status, budget, reps = (C.c_int * nb)(), (C.c_int * nb)(), (_lib.VerifyReport * nb)()
            prim = C.c_void_p(primaries.data_ptr() + 8 * b0 * vk.n_inputs * self.ring_words) if vk.n_inputs else None
            prf = C.c_void_p(proofs.data_ptr() + 8 * b0 * n_elems * self.level_words(K_lvl))
            _lib.check(fn(self.h, vk.h, K_lvl, nb, prim, prf, em, status, budget, reps, self.stream()))
            for b in range(nb):
                r = reps[b]
                res = None if status[b] != _lib.RS_OK else VerifyResult(bool(r.accepted), int(r.failed), tuple(int(x) for x in r.n_bad),
                                                                        int(r.first_check), int(r.first_limb), int(r.first_slot),
                                                                        int(r.lhs), int(r.rhs))
                out.append(BatchVerdict(res, status[b] == _lib.RS_ERR_NOISE, int(budget[b])))
        return out

    def groth16_verify_batch(self, vk, primaries, proofs, empties=None, level=None):
        """rs_groth16_verify_batch: B proofs ([3] encoding elements each) with their primary inputs against one key, as lists
        or stacked tensors [B][...]; empties: B lists of 3 flags, or None.  A list of B BatchVerdict: member b's result is the
        VerifyResult groth16_verify gives for it alone, or None with noise_spent set where that call raises RS_ERR_NOISE.
        level: every proof was switched to that many primes.  More than 64 members: successive calls."""
        return self._verify_batch(self.lib.rs_groth16_verify_batch, vk, "groth16", 3, primaries, proofs, empties, level)

    def rinocchio_verify_batch(self, vk, primaries, proofs, empties=None, level=None):
        """rs_rinocchio_verify_batch: as groth16_verify_batch with [9] elements and 9 flags per member; a member whose
        element 8 is EMPTY skips check 4, its neighbours do not."""
        return self._verify_batch(self.lib.rs_rinocchio_verify_batch, vk, "rinocchio", 9, primaries, proofs, empties, level)

    # ---- mod-switched encodings (ringsnark_amd/modswitch.h): level = number of leading primes an encoding still has
    def level_words(self, level=None):
        """words of one encoding element of `level` primes (None: the context's K)"""
        return self.enc_words if level is None else self.L * 2 * int(level) * self.N_enc

    def enc_mod_switch(self, enc, K_out, K_in=None):
        """EncodingElem::modswitch_inplace, K_in - K_out times (rs_enc_mod_switch): enc [..][L][2][K_in][N_enc] -> a new
        tensor [..][L][2][K_out][N_enc], an encoding of the context with primes Q[:K_out].  K_in: read off enc's shape.
        Needs no key.  The result decodes with enc_decode(sk, out, level=K_out)."""
        K_in = int(enc.shape[-2]) if K_in is None else int(K_in)
        assert enc.is_contiguous() and tuple(enc.shape[-4:]) == (self.L, 2, K_in, self.N_enc), tuple(enc.shape)
        count = self._count(enc, self.level_words(K_in))
        out = torch.empty(tuple(enc.shape[:-4]) + (self.L, 2, int(K_out), self.N_enc), dtype=torch.int64, device=self.device)
        _lib.check(self.lib.rs_enc_mod_switch(self.h, _ptr(enc), count, K_in, int(K_out), _ptr(out), self.stream()))
        return out

    # ---- generators (ringsnark_amd/keygen.h)
    KEYGEN_SEED_STRIDE = 1 << 40  # seeds=<int>: vector v of a key encodes from seed + v * 2^40 (disjoint streams for any length < 2^40)

    def _keygen_seeds(self, seeds, n):
        """n per-vector seeds in enc_encode's convention (element k of vector v: the oracle's stream seeds[v] * 65537 + k)."""
        if seeds is None:
            seeds = 1
        if isinstance(seeds, int):
            seeds = [seeds + v * self.KEYGEN_SEED_STRIDE for v in range(n)]
        assert len(seeds) == n, (len(seeds), n)
        return (C.c_uint64 * n)(*[(int(x) * 65537) % 2**64 for x in seeds])

    def _key_vector(self, count, host, seeded=False, packed=False):
        """seeded: the compact layout [count][L][K][N_enc] (ringsnark_amd/seeded.h); packed: [count][L][K][row_words]
        (ringsnark_amd/packed.h)"""
        if host:
            return self.host_alloc(max(count, 1) * (self.packed_words if packed else self.enc_words // 2 if seeded else self.enc_words))
        return self.packed_empty(count) if packed else self.c0_empty(count) if seeded else self.enc_empty(count)

    # ---- bit-packed seeded keys (ringsnark_amd/packed.h)
    @property
    def pack_bits(self):
        return int(self.lib.rs_enc_pack_bits(self.h))

    @property
    def packed_words(self):
        """words of one packed element, L K row_words"""
        return int(self.lib.rs_enc_packed_words(self.h))

    def packed_empty(self, *lead):
        return torch.empty(tuple(lead) + (self.L, self.K, self.packed_words // (self.L * self.K)), dtype=torch.int64, device=self.device)

    def enc_pack_c0(self, c0, want_bad=True):
        """rs_enc_pack_c0: compact elements [count][L][K][N_enc] -> (packed elements [count][L][K][row_words], the number of
        input words >= 2^w -- their low w bits are stored -- or None without want_bad)"""
        assert c0.is_contiguous()
        count = self._count(c0, self.enc_words // 2)
        out = self.packed_empty(count) if c0.dim() > 3 else self.packed_empty()
        bad = C.c_size_t(0)
        _lib.check(self.lib.rs_enc_pack_c0(self.h, _ptr(c0), count, _ptr(out), C.byref(bad) if want_bad else None, self.stream()))
        return out, (int(bad.value) if want_bad else None)

    def enc_unpack_c0(self, packed):
        """rs_enc_unpack_c0: packed elements -> compact elements"""
        assert packed.is_contiguous()
        count = self._count(packed, self.packed_words)
        out = self.c0_empty(count) if packed.dim() > 3 else self.c0_empty()
        _lib.check(self.lib.rs_enc_unpack_c0(self.h, _ptr(packed), count, _ptr(out), self.stream()))
        return out

    def enc_expand_packed(self, packed, pub_seed, first=0):
        """rs_enc_expand_packed: enc_expand_seeded on packed elements (c0 unpacked, c1 regenerated)"""
        assert packed.is_contiguous()
        count = self._count(packed, self.packed_words)
        out = self.enc_empty(count) if packed.dim() > 3 else self.enc_empty()
        _lib.check(self.lib.rs_enc_expand_packed(self.h, _ptr(packed), C.c_uint64((pub_seed * 65537) % 2**64), first, count, _ptr(out),
                                                 self.stream()))
        return out

    def c0_empty(self, *lead):
        return torch.empty(tuple(lead) + (self.L, self.K, self.N_enc), dtype=torch.int64, device=self.device)

    def _public_seeds(self, seeds, pub_seeds, lens, allow_shared_seeds):
        """(the public seeds of a seeded key in enc_encode's convention, their words for the C interface).  None: drawn from
        the `secrets` module, one 64-bit base and KEYGEN_SEED_STRIDE between the vectors.  A public stream that is also a
        private one hands the error polynomial to the prover (seeded.h): ValueError unless allow_shared_seeds (tests)."""
        n = len(lens)
        if pub_seeds is None:
            import secrets
            base = secrets.randbits(64)
            pub_seeds = [(base + v * self.KEYGEN_SEED_STRIDE) % 2**64 for v in range(n)]
        elif isinstance(pub_seeds, int):
            pub_seeds = [pub_seeds + v * self.KEYGEN_SEED_STRIDE for v in range(n)]
        pub_seeds = [int(x) for x in pub_seeds]
        assert len(pub_seeds) == n, (len(pub_seeds), n)
        words, priv = self._keygen_seeds(pub_seeds, n), self._keygen_seeds(seeds, n)
        meet = lambda a, la, b, lb: la and lb and ((b - a) % 2**64 < la or (a - b) % 2**64 < lb)
        if not allow_shared_seeds and any(meet(words[v], lens[v], priv[w], lens[w]) for v in range(n) for w in range(n)):
            raise ValueError("a public seed of a seeded key is also a private seed: the prover could compute the error polynomials "
                             "(pass allow_shared_seeds=True in tests only)")
        return pub_seeds, words

    def enc_expand_seeded(self, c0, pub_seed, first=0):
        """rs_enc_expand_seeded: compact elements c0 [count][L][K][N_enc] -> full elements [count][L][2][K][N_enc], c0 copied
        and c1 regenerated from the public stream of stored index first + i (pub_seed in enc_encode's convention).  With the
        c0 blocks of enc_encode(sk, rings, seed) and pub_seed = seed: those elements."""
        assert c0.is_contiguous()
        count = self._count(c0, self.enc_words // 2)
        out = self.enc_empty(count) if c0.dim() > 3 else self.enc_empty()
        _lib.check(self.lib.rs_enc_expand_seeded(self.h, _ptr(c0), C.c_uint64((pub_seed * 65537) % 2**64), first, count, _ptr(out),
                                                 self.stream()))
        return out

    def enc_encode_linear(self, sk, rows, seed, coefs=None):
        """rs_enc_encode_linear: E(sum_r coefs[r] * rows[r][k]) for every k; rows: one to three tensors [count][L][N], coefs:
        per term a ring element [L][N] or None (= 1).  With one term and no coefficient: the bytes of enc_encode(sk, rows[0], seed)."""
        n = len(rows)
        coefs = list(coefs) if coefs is not None else [None] * n
        count = self._count(rows[0], self.ring_words)
        assert all(self._count(r, self.ring_words) == count and r.is_contiguous() for r in rows)
        out = self.enc_empty(count)
        cp = (C.c_void_p * n)(*[None if c is None else c.data_ptr() for c in coefs])
        rp = (C.c_void_p * n)(*[r.data_ptr() for r in rows])
        _lib.check(self.lib.rs_enc_encode_linear(self.h, _ptr(sk), cp, rp, n, count, C.c_uint64((seed * 65537) % 2**64), _ptr(out),
                                                 self.stream()))
        return out

    def groth16_keygen(self, dcs, vk, seeds=None, host=False, tile=0, seeded=False, pub_seeds=None, allow_shared_seeds=False,
                       packed=False):
        """groth16::generator (groth16.tcc:5-66) on the device: the proving key of the trapdoor `vk` (the dict groth16_vk
        takes: s, alpha, beta, gamma, delta, sk), as the dict groth16_prove accepts.  seeds: None, one integer, or five
        (s_pows, delta_ts, delta_mid, alpha, beta) in enc_encode's convention; their ranges must not intersect.
        host: the three vectors are HostWords (a key larger than HBM), encoded in tiles of `tile` elements.
        seeded: a seeded key (ringsnark_amd/seeded.h) -- the three vectors compact [count][L][K][N_enc] (half the size), and
        "pub_seeds": the five public seeds their c1 halves are regenerated from (pub_seeds: None = drawn from `secrets`, one
        integer, or five); groth16_prove and enc_expand_seeded take them from the dict.
        packed (with seeded; ValueError otherwise): the three vectors bit-packed [count][L][K][row_words]
        (ringsnark_amd/packed.h), and "packed": True beside "pub_seeds"; the provers and msm dispatch on that mark."""
        if packed and not seeded:
            raise ValueError("packed=True needs seeded=True: a packed key is a seeded key (ringsnark_amd/packed.h)")
        t = {k: self._vk_part(vk[k]) for k in ("s", "alpha", "beta", "delta", "sk")}
        m, n_aux = dcs.m, dcs.n_vars - dcs.n_inputs
        if seeded:
            pub, pub_words = self._public_seeds(seeds, pub_seeds, [m + 1, m + 1, n_aux, 1, 1], allow_shared_seeds)
        self.sync()
        pk = dict(s_pows=self._key_vector(m + 1, host, seeded, packed), delta_ts=self._key_vector(m + 1, host, seeded, packed),
                  delta_mid=self._key_vector(n_aux, host, seeded, packed) if n_aux else None, alpha=self.enc_empty(), beta=self.enc_empty())
        addr = lambda v: None if v is None else (v.ptr if isinstance(v, HostWords) else v.data_ptr())
        members = (addr(pk["s_pows"]), addr(pk["delta_ts"]), addr(pk["delta_mid"]), pk["alpha"].data_ptr(), pk["beta"].data_ptr(),
                   1 if host else 0, tile)
        args = [self.h, dcs.h, _ptr(t["s"]), _ptr(t["alpha"]), _ptr(t["beta"]), _ptr(t["delta"]), _ptr(t["sk"]), self._keygen_seeds(seeds, 5)]
        if seeded:
            out = _lib.Groth16SeededKeyOut(*members)
            keygen = self.lib.rs_groth16_keygen_packed if packed else self.lib.rs_groth16_keygen_seeded
            _lib.check(keygen(*args, pub_words, C.byref(out), self.stream()))
            pk["pub_seeds"] = pub
            if packed:
                pk["packed"] = True
        else:
            out = _lib.Groth16KeyOut(*members)
            _lib.check(self.lib.rs_groth16_keygen(*args, C.byref(out), self.stream()))
        return pk

    def rinocchio_keygen(self, dcs, vk, seeds=None, host=False, tile=0, seeded=False, pub_seeds=None, allow_shared_seeds=False,
                         into=None, packed=False):
        """rinocchio::generator (rinocchio.tcc:5-72): the dict rinocchio_prove accepts, from the dict rinocchio_vk takes.
        seeds: s_pows, alpha_s_pows, beta_prods, beta_rv_ts, beta_rw_ts, beta_ry_ts.  seeded, pub_seeds, allow_shared_seeds:
        as in groth16_keygen (six public seeds).  into: a key this call returned for the same system, `host`, `seeded` and
        `packed`, whose buffers are written again instead of new ones (a host-resident key is tens of GiB of page-locked
        memory).  packed: as in groth16_keygen."""
        if packed and not seeded:
            raise ValueError("packed=True needs seeded=True: a packed key is a seeded key (ringsnark_amd/packed.h)")
        t = {k: self._vk_part(vk[k]) for k in ("s", "alpha", "beta", "r_v", "r_w", "r_y", "sk")}
        m, n_aux = dcs.m, dcs.n_vars - dcs.n_inputs
        if seeded:
            pub, pub_words = self._public_seeds(seeds, pub_seeds, [m + 1, m + 1, n_aux, 1, 1, 1], allow_shared_seeds)
        self.sync()
        pk = into if into is not None else dict(
            s_pows=self._key_vector(m + 1, host, seeded, packed), alpha_s_pows=self._key_vector(m + 1, host, seeded, packed),
            beta_prods=self._key_vector(n_aux, host, seeded, packed) if n_aux else None, beta_rv_ts=self.enc_empty(),
            beta_rw_ts=self.enc_empty(), beta_ry_ts=self.enc_empty())
        assert isinstance(pk["s_pows"], HostWords) == bool(host) and ("pub_seeds" in pk) == bool(seeded and into is not None)
        assert bool(pk.get("packed")) == bool(packed and into is not None)
        addr = lambda v: None if v is None else (v.ptr if isinstance(v, HostWords) else v.data_ptr())
        members = (addr(pk["s_pows"]), addr(pk["alpha_s_pows"]), addr(pk["beta_prods"]), pk["beta_rv_ts"].data_ptr(),
                   pk["beta_rw_ts"].data_ptr(), pk["beta_ry_ts"].data_ptr(), 1 if host else 0, tile)
        args = [self.h, dcs.h] + [_ptr(t[k]) for k in ("s", "alpha", "beta", "r_v", "r_w", "r_y", "sk")] + [self._keygen_seeds(seeds, 6)]
        if seeded:
            out = _lib.RinocchioSeededKeyOut(*members)
            keygen = self.lib.rs_rinocchio_keygen_packed if packed else self.lib.rs_rinocchio_keygen_seeded
            _lib.check(keygen(*args, pub_words, C.byref(out), self.stream()))
            pk["pub_seeds"] = pub
            if packed:
                pk["packed"] = True
        else:
            out = _lib.RinocchioKeyOut(*members)
            _lib.check(self.lib.rs_rinocchio_keygen(*args, C.byref(out), self.stream()))
        return pk

    # ---- 8(f) f4
    def enc_serialize(self, enc, empty=None, level=None):
        """Encoding elements (a proof, a key vector) -> bytes in the wire format of ringsnark_amd.h.
        level: enc has that many primes (enc_mod_switch); the stream is what a context on Q[:level] writes."""
        import numpy as np
        count = self._count(enc, self.level_words(level))
        if level is None:
            size = self.lib.rs_enc_wire_size(self.h, count)
        else:
            size = self.lib.rs_enc_wire_size_level(self.h, int(level), count)
            if size == 0:
                raise _lib.RsError(_lib.RS_ERR_INVALID, "level out of range: 1 <= K_lvl <= K")
        buf = np.empty(size, dtype=np.uint8)
        em = None
        if empty is not None:
            em = np.ascontiguousarray(empty, dtype=np.uint8)
            assert em.size == count
        emp = None if em is None else em.ctypes.data_as(_lib.u8p)
        if level is None:
            _lib.check(self.lib.rs_enc_serialize(self.h, _ptr(enc), emp, count, buf.ctypes.data_as(C.c_void_p), size, self.stream()))
        else:
            _lib.check(self.lib.rs_enc_serialize_level(self.h, int(level), _ptr(enc), emp, count, buf.ctypes.data_as(C.c_void_p), size,
                                                       self.stream()))
        return buf.tobytes()

    def enc_deserialize(self, data, level=None):
        """bytes -> (encodings [count][L][2][K][N_enc] on the device, empty flags).  Validates the stream.
        level: 0 accepts a stream of any level of this context, K_lvl only that one (rs_enc_deserialize_level); returns
        (encodings [count][L][2][K_lvl][N_enc], empty flags, K_lvl)."""
        import numpy as np
        buf = np.frombuffer(data, dtype=np.uint8)
        cnt = C.c_size_t(0)
        if level is not None:
            found = C.c_int(0)
            _lib.check(self.lib.rs_enc_deserialize_level(self.h, buf.ctypes.data_as(C.c_void_p), buf.size, None, None, 0, C.byref(cnt),
                                                         C.byref(found), self.stream()))
            if level and found.value != level:
                raise _lib.RsError(_lib.RS_ERR_INVALID, "stream of level %d, expected level %d" % (found.value, level))
            out = torch.empty((cnt.value, self.L, 2, found.value, self.N_enc), dtype=torch.int64, device=self.device)
            em = np.zeros(cnt.value, dtype=np.uint8)
            _lib.check(self.lib.rs_enc_deserialize_level(self.h, buf.ctypes.data_as(C.c_void_p), buf.size, _ptr(out),
                                                         em.ctypes.data_as(_lib.u8p), cnt.value, C.byref(cnt), C.byref(found), self.stream()))
            return out, em, found.value
        _lib.check(self.lib.rs_enc_deserialize(self.h, buf.ctypes.data_as(C.c_void_p), buf.size, None, None, 0, C.byref(cnt),
                                               self.stream()))
        out = self.enc_empty(cnt.value)
        em = np.zeros(cnt.value, dtype=np.uint8)
        _lib.check(self.lib.rs_enc_deserialize(self.h, buf.ctypes.data_as(C.c_void_p), buf.size, _ptr(out),
                                               em.ctypes.data_as(_lib.u8p), cnt.value, C.byref(cnt), self.stream()))
        return out, em

    # ---- 8(f) f2 / f3
    def enc_decode(self, sk, enc, level=None):
        """EncodingElem::decode (seal_ring.tcc:435-477): sk [K][N_enc] NTT form -> ring elements.  Raises
        RsError(RS_ERR_NOISE, "ciphertext #i has remaining noise budget 0 <= 0") like the reference's decoding_error
        (seal_ring.tcc:446-454) when a ciphertext's invariant noise budget is spent.
        level: enc [..][L][2][level][N_enc] was switched to that many primes (rs_enc_decode_level)."""
        count = self._count(enc, self.level_words(level))
        out = self.ring_empty(count) if enc.dim() > 4 else self.ring_empty()
        if level is None:
            _lib.check(self.lib.rs_enc_decode(self.h, _ptr(sk), _ptr(enc), count, _ptr(out), self.stream()))
        else:
            _lib.check(self.lib.rs_enc_decode_level(self.h, int(level), _ptr(sk), _ptr(enc), count, _ptr(out), self.stream()))
        return out

    def enc_noise_budget(self, sk, enc, level=None):
        """Decryptor::invariant_noise_budget of every ciphertext (bits; 0 = spent): int array [count][L].
        level: as in enc_decode (rs_enc_noise_budget_level)."""
        count = self._count(enc, self.level_words(level))
        out = (C.c_int * (count * self.L))()
        if level is None:
            _lib.check(self.lib.rs_enc_noise_budget(self.h, _ptr(sk), _ptr(enc), count, out, self.stream()))
        else:
            _lib.check(self.lib.rs_enc_noise_budget_level(self.h, int(level), _ptr(sk), _ptr(enc), count, out, self.stream()))
        return np.array(out, dtype=np.int64).reshape(count, self.L)

    def enc_encode(self, sk, rings, seed):
        """EncodingElem::encode (seal_ring.tcc:324-359); element k uses the oracle's stream seed*65537 + k."""
        count = self._count(rings, self.ring_words)
        out = self.enc_empty(count) if rings.dim() > 2 else self.enc_empty()
        _lib.check(self.lib.rs_enc_encode(self.h, _ptr(sk), _ptr(rings), count, C.c_uint64((seed * 65537) % 2**64), _ptr(out),
                                          self.stream()))
        return out

    # ---- a9
    def inner_product(self, encs, rings, kinds=None, want_used=True):
        """EncodingElem::inner_product.  Returns (out, used); used == 0 <=> EMPTY element."""
        T = self._count(rings, self.ring_words)
        assert self._count(encs, self.enc_words) == T
        out = self.enc_empty()
        used = C.c_size_t(0)
        kp = None
        if kinds is not None:
            kinds = np.ascontiguousarray(kinds, dtype=np.uint8)
            kp = kinds.ctypes.data_as(_lib.u8p)
        _lib.check(self.lib.rs_inner_product(self.h, _ptr(encs), _ptr(rings), kp, T, _ptr(out),
                                             C.byref(used) if want_used else None, self.stream()))
        return out, int(used.value)

    def msm(self, crs_list, vecs, n_groups, want_used=False, crs_len=None, window=0, pub_seeds=None, packed=False):
        """vecs: list of (coeff tensor [T][L][N], kinds or None, group) or, for a SLOT-CONSTANT vector (one value per
        (term, limb) in every slot: coefficients_for_Z), (tensor [T][L], kinds, group, True).  window != 0: the CRS tensors hold
        `window` elements and logical element t is read from t % window (crs_len = logical length).
        CRS vectors given as HostWords (host_alloc) are streamed from host memory (rs_msm_hostkey).
        pub_seeds (one per CRS vector, as a seeded key's "pub_seeds" holds them): the CRS vectors are COMPACT (rs_msm_seeded);
        packed (with pub_seeds, as a packed key's "packed" mark): they are bit-packed (rs_msm_packed)."""
        if packed and pub_seeds is None:
            raise ValueError("packed=True needs pub_seeds: a packed key is a seeded key")
        n_crs = len(crs_list)
        on_host = isinstance(crs_list[0], HostWords)
        assert all(isinstance(c, HostWords) == on_host for c in crs_list)
        key_words = self.enc_words if pub_seeds is None else self.packed_words if packed else self.enc_words // 2
        if crs_len is None:
            crs_len = crs_list[0].words // key_words if on_host else self._count(crs_list[0], key_words)
        crs = (C.c_void_p * n_crs)(*[(c.ptr if on_host else c.data_ptr()) for c in crs_list])
        mv = (_lib.MsmVec * len(vecs))()
        keep = []
        for k, vec in enumerate(vecs):
            coeff, kinds, group = vec[:3]
            slot_const = len(vec) > 3 and bool(vec[3])
            assert coeff.is_contiguous()
            mv[k].d_coeff = coeff.data_ptr()
            mv[k].T = self._count(coeff, self.L if slot_const else self.ring_words)
            mv[k].group = group
            mv[k].slot_const = 1 if slot_const else 0
            if kinds is not None:
                kk = np.ascontiguousarray(kinds, dtype=np.uint8)
                keep.append(kk)
                mv[k].h_kinds = kk.ctypes.data_as(_lib.u8p)
        out = self.enc_empty(n_crs, n_groups)
        used = (C.c_size_t * len(vecs))()
        if pub_seeds is not None:
            assert len(pub_seeds) == n_crs
            fn = self.lib.rs_msm_packed if packed else self.lib.rs_msm_seeded
            _lib.check(fn(self.h, crs, self._keygen_seeds(list(pub_seeds), n_crs), 1 if on_host else 0, n_crs, crs_len,
                          window, mv, len(vecs), n_groups, _ptr(out), used if want_used else None, self.stream()))
            return out, [int(u) for u in used]
        fn = self.lib.rs_msm_hostkey if on_host else self.lib.rs_msm
        _lib.check(fn(self.h, crs, n_crs, crs_len, window, mv, len(vecs), n_groups, _ptr(out), used if want_used else None, self.stream()))
        return out, [int(u) for u in used]

    # ---- a10-a14
    def r1cs(self, cs: R1CS):
        return DeviceR1CS(self, cs)

    def r1cs_evaluate(self, dcs, which, mode, assignment):
        out = self.ring_empty(dcs.m)
        _lib.check(self.lib.rs_r1cs_evaluate(self.h, dcs.h, which, mode, _ptr(assignment), _ptr(out), self.stream()))
        return out

    def r1cs_check(self, dcs, assignment, want_flags=False):
        """r1cs_constraint_system::is_satisfied on the device (rs_r1cs_check): one fused pass over the FULL assignment
        [n_vars][L][N].  Returns an R1csCheck (satisfied, n_violated, first_row, first_limb, first_slot, a, b, c);
        want_flags: .flags is a uint8 tensor [m], 1 = constraint violated in some slot."""
        assert self._count(assignment, self.ring_words) == dcs.n_vars, "the check reads every row of the assignment"
        flags = torch.empty(dcs.m, dtype=torch.uint8, device=self.device) if want_flags else None
        rep = _lib.R1csReport()
        _lib.check(self.lib.rs_r1cs_check(self.h, dcs.h, _ptr(assignment), None if flags is None else C.c_void_p(flags.data_ptr()),
                                          C.byref(rep), self.stream()))
        return R1csCheck(int(rep.n_violated), int(rep.first_row), int(rep.first_limb), int(rep.first_slot), int(rep.a), int(rep.b),
                         int(rep.c), flags)

    def r1cs_solve_plan(self, dcs, given):
        """The schedule that completes an assignment of `dcs` from the `given` wires (an iterable of 0-based variables or a
        bool mask [n_vars]): rs_r1cs_solve_plan_create.  A plan with unsolved wires is still a plan; .info says what is
        missing and why."""
        return SolvePlan(self, dcs, given)

    def r1cs_solve(self, plan, assignment, mode="auto", allow_partial=False):
        """Fills the rows of the solved wires of `assignment` [n_vars][L][N] in place (rs_r1cs_solve) and returns
        SolveStats(level_launches, walk_launches).  Rows that are neither given nor solved are never read and stay as they
        are.  With unsolved wires it raises ValueError unless allow_partial."""
        assert self._count(assignment, self.ring_words) == plan.dcs.n_vars, "the solver addresses every row of the assignment"
        i = plan.info
        if i.n_unsolved and not allow_partial:
            raise ValueError("the given wires do not determine the assignment: %d of %d variables unsolved, first unsolved variable %d; "
                             "first blocked constraint %d: %s" % (i.n_unsolved, plan.dcs.n_vars, i.first_unsolved, i.first_blocked,
                                                                  SOLVE_BLOCKED[i.blocked_reason]))
        stats = _lib.SolveStats()
        _lib.check(self.lib.rs_r1cs_solve(self.h, plan.h, _ptr(assignment), SOLVE_MODES[mode], C.byref(stats), self.stream()))
        return SolveStats(int(stats.level_launches), int(stats.walk_launches))

    def r1cs_solve_batch(self, plan, assignments, mode="auto", allow_partial=False):
        """r1cs_solve for B assignments (a list of device tensors [n_vars][L][N], 1 <= B <= 8, no two overlapping) of one
        plan in one pass over the schedule and the system (rs_r1cs_solve_batch): every member ends word for word as
        r1cs_solve leaves it.  Returns SolveStats of the whole batch, equal to those of one r1cs_solve call."""
        assignments = list(assignments)
        for a in assignments:
            assert self._count(a, self.ring_words) == plan.dcs.n_vars, "the solver addresses every row of the assignment"
        i = plan.info
        if i.n_unsolved and not allow_partial:
            raise ValueError("the given wires do not determine the assignment: %d of %d variables unsolved, first unsolved variable %d; "
                             "first blocked constraint %d: %s" % (i.n_unsolved, plan.dcs.n_vars, i.first_unsolved, i.first_blocked,
                                                                  SOLVE_BLOCKED[i.blocked_reason]))
        B = len(assignments)
        ptrs = (C.c_void_p * max(B, 1))(*[a.data_ptr() for a in assignments])
        stats = _lib.SolveStats()
        _lib.check(self.lib.rs_r1cs_solve_batch(self.h, plan.h, B, ptrs, SOLVE_MODES[mode], C.byref(stats), self.stream()))
        return SolveStats(int(stats.level_launches), int(stats.walk_launches))

    def r1cs_hint_plan(self, dcs, given, hints):
        """The schedule that completes an assignment of `dcs` from the `given` wires and the declared `hints` (a list of
        ringsnark_amd.r1cs.Hint): rs_r1cs_hint_plan_create.  A plan with unsolved wires or blocked hints is still a plan;
        .info says what is missing and why.  A hint the library refuses raises RsError."""
        return HintPlan(self, dcs, given, hints)

    def r1cs_solve_hinted(self, plan, assignment, mode="auto", allow_partial=False, want_report=True):
        """Fills the rows of the wires that the constraints and the hints of `plan` determine in `assignment` [n_vars][L][N]
        in place (rs_r1cs_solve_hinted).  Returns (HintSolveStats, HintReport), or (HintSolveStats, None) with
        want_report=False: enqueued only, nothing is downloaded.  Bad bits and zero sources are answers in the report, not
        errors.  With unsolved wires it raises ValueError unless allow_partial, as r1cs_solve does."""
        assert self._count(assignment, self.ring_words) == plan.dcs.n_vars, "the solver addresses every row of the assignment"
        i = plan.info
        if i.n_unsolved and not allow_partial:
            raise ValueError("the given wires and the hints do not determine the assignment: %d of %d variables unsolved, first unsolved "
                             "variable %d; first blocked constraint %d: %s; %d hints never ready" % (
                                 i.n_unsolved, plan.dcs.n_vars, i.first_unsolved, i.first_blocked, SOLVE_BLOCKED[i.blocked_reason],
                                 i.n_hints_blocked))
        stats, rep = _lib.HintStats(), _lib.HintReport()
        _lib.check(self.lib.rs_r1cs_solve_hinted(self.h, plan.h, _ptr(assignment), SOLVE_MODES[mode], C.byref(stats),
                                                 C.byref(rep) if want_report else None, self.stream()))
        stats = HintSolveStats(int(stats.level_launches), int(stats.walk_launches), int(stats.hint_launches))
        if not want_report:
            return stats, None
        return stats, HintReport(int(rep.n_bits_bad), int(rep.bad_hint), int(rep.bad_limb), int(rep.bad_slot), int(rep.n_zero),
                                 int(rep.zero_hint), int(rep.zero_limb), int(rep.zero_slot))

    def r1cs_check_batch(self, dcs, assignments, want_flags=False):
        """r1cs_check for B FULL assignments (1 <= B <= 8; members may alias) in one pass over the three matrices
        (rs_r1cs_check_batch): one main and one epilogue launch, one download.  Returns a list of R1csCheck, member b's equal to
        r1cs_check of it; want_flags: .flags of member b is row b of one uint8 tensor [B][m]."""
        assignments = list(assignments)
        for a in assignments:
            assert self._count(a, self.ring_words) == dcs.n_vars, "the check reads every row of the assignment"
        B = len(assignments)
        ptrs = (C.c_void_p * max(B, 1))(*[a.data_ptr() for a in assignments])
        flags = torch.empty((max(B, 1), dcs.m), dtype=torch.uint8, device=self.device) if want_flags else None
        reps = (_lib.R1csReport * max(B, 1))()
        _lib.check(self.lib.rs_r1cs_check_batch(self.h, dcs.h, B, ptrs, None if flags is None else C.c_void_p(flags.data_ptr()), reps,
                                                self.stream()))
        return [R1csCheck(int(r.n_violated), int(r.first_row), int(r.first_limb), int(r.first_slot), int(r.a), int(r.b), int(r.c),
                          None if flags is None else flags[b]) for b, r in enumerate(reps[:B])]

    def ring_bit_decompose(self, x, nbits, out=None, x_stride=1, bits_stride=None, want_report=True):
        """The bit rows of ring elements whose slots hold one integer below 2^nbits in every limb (rs_ring_bit_decompose).
        x: a tensor whose element e is the ring element at x_stride * e ring elements (x_stride = 1: [count][L][N]); bit k
        of element e is written to ring element e * bits_stride + k of `out` (default bits_stride = nbits; out = None: a
        new [count][nbits][L][N]).  x and out may be views of one assignment as long as no x row is a bit row.
        Returns (out, BitsResult), or (out, None) with want_report=False: enqueued only, nothing is downloaded."""
        bits_stride = nbits if bits_stride is None else bits_stride
        assert x_stride >= 1, "x_stride must be at least 1"
        count = (self._count(x, self.ring_words) - 1) // x_stride + 1 if x.numel() else 0
        if out is None:
            assert bits_stride == nbits, "a strided output needs `out`"
            out = self.ring_empty(count, nbits)
        elif count:
            need = (count - 1) * bits_stride + nbits
            assert self._count(out, self.ring_words) >= need, "out holds fewer than (count - 1) * bits_stride + nbits ring elements"
        rep = _lib.BitsReport()
        _lib.check(self.lib.rs_ring_bit_decompose(self.h, _ptr(x), x_stride, count, nbits, _ptr(out), bits_stride,
                                                  C.byref(rep) if want_report else None, self.stream()))
        if not want_report:
            return out, None
        return out, BitsResult(*[int(getattr(rep, k)) for k, _ in _lib.BitsReport._fields_])

    def plaintext_check_fill_bits(self, assignment, cs_or_logT, count, constants=False, want_report=True):
        """Fills the bit rows of a plaintext_check_r1cs assignment [n_vars][L][N] in place from its x rows (block p: rows
        b_0 .. b_{logT-1}, x): one strided rs_ring_bit_decompose, x_stride = bits_stride = logT + 1.  The circuit is given
        as the R1CS itself or as logT and `constants`.  Returns the report."""
        logT, first = plaintext_check_layout(cs_or_logT, count, constants)
        rows = assignment.view(-1, self.L, self.N)
        assert rows.shape[0] == first + count * (logT + 1), "not an assignment of %d blocks of logT = %d" % (count, logT)
        _, rep = self.ring_bit_decompose(rows[first + logT:], logT, out=rows[first:], x_stride=logT + 1, bits_stride=logT + 1,
                                         want_report=want_report)
        return rep

    def ring_inv_or_zero(self, x, num=None, out=None, x_stride=1, num_stride=1, out_stride=1, want_report=True):
        """The slotwise inverse-or-zero of ring elements (rs_ring_inv_or_zero): x^-1 where a slot is non-zero, 0 where it is
        zero; with `num`, num * x^-1.  x: a tensor whose element e is the ring element at x_stride * e ring elements
        (x_stride = 1: [count][L][N]); likewise num and out (out = None: a new [count][L][N]).  The three may be views of
        one assignment as long as no x or num row is an output row; num may be x.
        Returns (out, InvReport), or (out, None) with want_report=False: enqueued only, nothing is downloaded."""
        assert x_stride >= 1 and num_stride >= 1 and out_stride >= 1, "strides must be at least 1"
        count = (self._count(x, self.ring_words) - 1) // x_stride + 1 if x.numel() else 0
        if num is not None and count:
            assert self._count(num, self.ring_words) >= (count - 1) * num_stride + 1, "num holds fewer than (count - 1) * num_stride + 1 ring elements"
        if out is None:
            assert out_stride == 1, "a strided output needs `out`"
            out = self.ring_empty(count)
        elif count:
            assert self._count(out, self.ring_words) >= (count - 1) * out_stride + 1, "out holds fewer than (count - 1) * out_stride + 1 ring elements"
        rep = _lib.InvReport()
        _lib.check(self.lib.rs_ring_inv_or_zero(self.h, _ptr(x), x_stride, _ptr(num), num_stride, count, _ptr(out), out_stride,
                                                C.byref(rep) if want_report else None, self.stream()))
        if not want_report:
            return out, None
        return out, InvReport(*[int(getattr(rep, k)) for k, _ in _lib.InvReport._fields_])

    def is_zero_fill(self, assignment, count, want_report=True):
        """Fills the inv rows of an is_zero_r1cs assignment [1 + 3 count][L][N] in place from its x rows (block p: rows
        x, inv, z after the row of `one`): one strided rs_ring_inv_or_zero, x_stride = out_stride = 3.  Returns the report."""
        rows = assignment.view(-1, self.L, self.N)
        assert rows.shape[0] == 1 + 3 * count, "not an assignment of %d is-zero blocks" % count
        _, rep = self.ring_inv_or_zero(rows[1:2 + 3 * (count - 1)], out=rows[2:], x_stride=3, out_stride=3, want_report=want_report)
        return rep

    def division_fill(self, assignment, count, want_report=True):
        """Fills the binv and y rows of a division_r1cs assignment [1 + 4 count][L][N] in place from its a and b rows (block
        p: rows a, b, binv, y after the row of `one`): two strided rs_ring_inv_or_zero of stride 4, binv from b, then y from
        b with num = a.  Returns the two reports."""
        rows = assignment.view(-1, self.L, self.N)
        assert rows.shape[0] == 1 + 4 * count, "not an assignment of %d division blocks" % count
        last = 4 * (count - 1)
        b = rows[2:3 + last]
        _, rep_binv = self.ring_inv_or_zero(b, out=rows[3:], x_stride=4, out_stride=4, want_report=want_report)
        _, rep_y = self.ring_inv_or_zero(b, num=rows[1:2 + last], out=rows[4:], x_stride=4, num_stride=4, out_stride=4, want_report=want_report)
        return rep_binv, rep_y

    def _require_satisfied(self, dcs, assignment, report=None):
        r = self.r1cs_check(dcs, assignment) if report is None else report
        if not r.satisfied:
            raise ValueError("assignment does not satisfy the constraint system: %d of %d constraints violated, first constraint %d "
                             "at limb %d, slot %d (a = %d, b = %d, c = %d)"
                             % (r.n_violated, dcs.m, r.first_row, r.first_limb, r.first_slot, r.a, r.b, r.c))

    def interpolate(self, y):
        n = self._count(y, self.ring_words)
        out = torch.empty_like(y)
        _lib.check(self.lib.rs_interpolate(self.h, _ptr(y), _ptr(out), n, self.stream()))
        return out

    def witness_map(self, dcs, assignment, d1=None, d2=None, d3=None, want=("A_io", "B_io", "C_io", "A_mid", "B_mid", "C_mid", "H"),
                    rows=None):
        """rows: {name: (lo, hi)} -- keep only rows [lo, hi) of those outputs (rs_witness_map_rows: a rank of a limb
        group keeps the rows of its term range); outputs not named keep every row."""
        m = dcs.m
        names = ("A_io", "B_io", "C_io", "A_mid", "B_mid", "C_mid", "H")
        if rows is not None:
            full = {k: (0, m + 1 if k == "H" else m) for k in names}
            rr = {k: tuple(int(x) for x in rows.get(k, full[k])) for k in names}
            for a, b in (("A_io", "A_mid"), ("B_io", "B_mid"), ("C_io", "C_mid")):  # one pass writes both: same range
                if (a in rows) != (b in rows):  # a range given for one of the pair holds for both
                    rr[a] = rr[b] = rr[a if a in rows else b]
                assert rr[a] == rr[b] or a not in want or b not in want, (a, b, rr[a], rr[b])
                if a not in want:
                    rr[a] = rr[b]
                if b not in want:
                    rr[b] = rr[a]
            o = {k: (torch.empty((rr[k][1] - rr[k][0], self.L, self.N), dtype=torch.int64, device=self.device) if k in want else None) for k in names}
            flat = (C.c_size_t * 14)(*[x for k in names for x in rr[k]])
            Z = np.zeros((self.L, m + 1), dtype=np.uint64)
            _lib.check(self.lib.rs_witness_map_rows(
                self.h, dcs.h, _ptr(assignment), _ptr(d1), _ptr(d2), _ptr(d3), flat, _ptr(o["A_io"]), _ptr(o["B_io"]), _ptr(o["C_io"]),
                _ptr(o["A_mid"]), _ptr(o["B_mid"]), _ptr(o["C_mid"]), _ptr(o["H"]), Z.ctypes.data_as(_lib.u64p), self.stream()))
            o["Z"] = Z
            return o
        o = {}
        for k in ("A_io", "B_io", "C_io", "A_mid", "B_mid", "C_mid"):
            o[k] = self.ring_empty(m) if k in want else None
        o["H"] = self.ring_empty(m + 1) if "H" in want else None
        Z = np.zeros((self.L, m + 1), dtype=np.uint64)
        _lib.check(self.lib.rs_witness_map(
            self.h, dcs.h, _ptr(assignment), _ptr(d1), _ptr(d2), _ptr(d3), _ptr(o["A_io"]), _ptr(o["B_io"]), _ptr(o["C_io"]),
            _ptr(o["A_mid"]), _ptr(o["B_mid"]), _ptr(o["C_mid"]), _ptr(o["H"]), Z.ctypes.data_as(_lib.u64p), self.stream()))
        o["Z"] = Z
        return o

    def witness_map_slots(self, dcs, assignment, slot0, nslots, d1=None, d2=None, d3=None,
                          want=("A_io", "B_io", "C_io", "A_mid", "B_mid", "C_mid", "H")):
        """The witness map on slots [slot0, slot0+nslots) of every limb; outputs compact [t][L][nslots]."""
        m = dcs.m
        o = {}
        mk = lambda rows: torch.empty((rows, self.L, nslots), dtype=torch.int64, device=self.device)
        for k in ("A_io", "B_io", "C_io", "A_mid", "B_mid", "C_mid"):
            o[k] = mk(m) if k in want else None
        o["H"] = mk(m + 1) if "H" in want else None
        Z = np.zeros((self.L, m + 1), dtype=np.uint64)
        _lib.check(self.lib.rs_witness_map_slots(
            self.h, dcs.h, _ptr(assignment), _ptr(d1), _ptr(d2), _ptr(d3), slot0, nslots, _ptr(o["A_io"]), _ptr(o["B_io"]),
            _ptr(o["C_io"]), _ptr(o["A_mid"]), _ptr(o["B_mid"]), _ptr(o["C_mid"]), _ptr(o["H"]), Z.ctypes.data_as(_lib.u64p),
            self.stream()))
        o["Z"] = Z
        return o

    # ---- a11: util/polynomials.tcc:62-81
    def _poly(self, fn, a, b, rows, out=None):
        """out: optional caller buffer of the nominal row count (the library zeroes the rows beyond the result)."""
        na, nb = self._count(a, self.ring_words), self._count(b, self.ring_words)
        if out is None:
            out = torch.empty((max(rows(na, nb), 1), self.L, self.N), dtype=torch.int64, device=self.device)
        assert out.shape[0] >= max(rows(na, nb), 0)
        n = C.c_size_t(0)
        _lib.check(fn(self.h, _ptr(a) if na else None, na, _ptr(b) if nb else None, nb, _ptr(out), C.byref(n), self.stream()))
        return out[:n.value]

    def poly_multiply(self, a, b, out=None):
        """multiply(x, y): coefficient vectors [n][L][N]; the result is normalised like Boost's polynomial."""
        return self._poly(self.lib.rs_poly_multiply, a, b, lambda na, nb: na + nb - 1 if na and nb else 0, out)

    def poly_add(self, a, b, out=None):
        return self._poly(self.lib.rs_poly_add, a, b, lambda na, nb: max(na, nb), out)

    def poly_divide(self, num, den, out=None):
        """divide(numerator, denominator): the quotient; RsError(RS_ERR_NOT_INVERTIBLE) unless the divisor's leading
        coefficient is a unit."""
        return self._poly(self.lib.rs_poly_divide, num, den, lambda nn, nd: nn - nd + 1, out)

    # ---- a15 / a16
    def host_alloc(self, words):
        """Page-locked host memory of `words` uint64 (rs_host_alloc): where a proving key larger than HBM lives."""
        return HostWords(self, words)

    def _kinds(self, kinds, n):
        """per-wire representation (RS_KIND_*) as a host uint8 array, or (None, None)"""
        if kinds is None:
            return None, None
        k = np.ascontiguousarray(kinds, dtype=np.uint8)
        assert k.shape == (n,), (k.shape, n)
        return k, k.ctypes.data_as(_lib.u8p)

    def groth16_prove(self, dcs, pk, assignment, want_empty=True, window=0, kinds=None, check=False):
        """pk: dict s_pows, delta_ts, delta_mid, alpha, beta (CUDA tensors).  window != 0: the key vectors hold
        `window` elements each, element t read from t % window (tiled synthetic key, ringsnark_amd.h).
        Key VECTORS given as HostWords: a host-resident key, streamed tile by tile (rs_groth16_pk.host_key).
        kinds [n_vars]: RS_KIND_ONE for assignment wires held as RingElem Scalar 1 (rs_groth16_prove_kinds).
        check: test the reference's precondition first (r1cs_check; groth16.tcc:74) and raise ValueError, naming the first
        violated constraint, limb and slot, for an assignment that does not satisfy the system."""
        if check:
            self._require_satisfied(dcs, assignment)
        s, seeded = self._groth16_key(pk, window)
        proof = self.enc_empty(3)
        empty = (C.c_int * 3)()
        keep, kp = self._kinds(kinds, dcs.n_vars)
        prove = self._prover(pk, "rs_groth16_prove_kinds", "rs_groth16_prove_seeded", "rs_groth16_prove_packed")
        _lib.check(prove(self.h, dcs.h, C.byref(s), _ptr(assignment), kp, _ptr(proof), empty if want_empty else None, self.stream()))
        return proof, [int(e) for e in empty]

    def rinocchio_prove(self, dcs, pk, assignment, d1=None, d2=None, d3=None, window=0, kinds=None, check=False):
        """check: as in groth16_prove (the reference asserts satisfaction at r1cs_to_qrp.tcc:156)."""
        if check:
            self._require_satisfied(dcs, assignment)
        s, seeded = self._rinocchio_key(pk, window)
        proof = self.enc_empty(9)
        empty = (C.c_int * 9)()
        keep, kp = self._kinds(kinds, dcs.n_vars)
        prove = self._prover(pk, "rs_rinocchio_prove_kinds", "rs_rinocchio_prove_seeded", "rs_rinocchio_prove_packed")
        _lib.check(prove(self.h, dcs.h, C.byref(s), _ptr(assignment), kp, _ptr(d1), _ptr(d2), _ptr(d3), _ptr(proof), empty, self.stream()))
        return proof, [int(e) for e in empty]

    def _prover(self, pk, full, seeded, packed):
        """the entry point for a key dictionary: "packed" (with "pub_seeds") a packed key, "pub_seeds" a seeded key"""
        if pk.get("packed"):
            assert "pub_seeds" in pk, "a packed key is a seeded key"
            return getattr(self.lib, packed)
        return getattr(self.lib, seeded if "pub_seeds" in pk else full)

    # ---- batched proving (include/ringsnark_amd/batch.h)
    def _groth16_key(self, pk, window):
        """(key struct, seeded) of a key dictionary; seeded: it has "pub_seeds" (groth16_keygen(seeded=True)) and compact vectors"""
        host_key = isinstance(pk["s_pows"], HostWords)
        addr = lambda v: None if v is None else (v.ptr if isinstance(v, HostWords) else v.data_ptr())
        assert all(isinstance(pk[k], HostWords) == host_key for k in ("s_pows", "delta_ts") + (("delta_mid",) if pk.get("delta_mid") is not None else ()))
        if "pub_seeds" in pk:
            return _lib.Groth16PKSeeded(addr(pk["s_pows"]), addr(pk["delta_ts"]), addr(pk.get("delta_mid")),
                                        (C.c_uint64 * 3)(*self._keygen_seeds(list(pk["pub_seeds"][:3]), 3)), pk["alpha"].data_ptr(),
                                        pk["beta"].data_ptr(), window, 1 if host_key else 0), True
        return _lib.Groth16PK(addr(pk["s_pows"]), addr(pk["delta_ts"]), addr(pk.get("delta_mid")), pk["alpha"].data_ptr(),
                              pk["beta"].data_ptr(), window, 1 if host_key else 0), False

    def _rinocchio_key(self, pk, window):
        host_key = isinstance(pk.get("s_pows"), HostWords)
        g = lambda k: None if pk.get(k) is None else (pk[k].ptr if isinstance(pk[k], HostWords) else pk[k].data_ptr())
        if "pub_seeds" in pk:
            return _lib.RinocchioPKSeeded(g("s_pows"), g("alpha_s_pows"), g("beta_prods"),
                                          (C.c_uint64 * 3)(*self._keygen_seeds(list(pk["pub_seeds"][:3]), 3)), g("beta_rv_ts"),
                                          g("beta_rw_ts"), g("beta_ry_ts"), window, 1 if host_key else 0), True
        return _lib.RinocchioPK(g("s_pows"), g("alpha_s_pows"), g("beta_prods"), g("beta_rv_ts"), g("beta_rw_ts"), g("beta_ry_ts"),
                                window, 1 if host_key else 0), False

    def _batch_args(self, dcs, assignments, kinds, check):
        """(B, host array of the members' device pointers, kinds array [B][n_vars] or None and its pointer)"""
        assignments = list(assignments)
        B = len(assignments)
        if check:
            # one pass over the system for the whole batch (a batch the provers refuse anyway: member by member, as before)
            reports = self.r1cs_check_batch(dcs, assignments) if 1 <= B <= 8 else [None] * B
            for b, a in enumerate(assignments):
                try:
                    self._require_satisfied(dcs, a, reports[b])
                except ValueError as e:
                    raise ValueError("batch member %d: %s" % (b, e)) from None
        ptrs = (C.c_void_p * max(B, 1))(*[a.data_ptr() for a in assignments])
        if kinds is None:
            return B, ptrs, None, None
        k = np.ascontiguousarray(np.stack([np.zeros(dcs.n_vars, dtype=np.uint8) if x is None else np.asarray(x, dtype=np.uint8)
                                           for x in kinds]))
        assert k.shape == (B, dcs.n_vars), (k.shape, B, dcs.n_vars)
        return B, ptrs, k, k.ctypes.data_as(_lib.u8p)

    def groth16_prove_batch(self, dcs, pk, assignments, window=0, kinds=None, check=False):
        """Proves the B assignments (a list of device tensors [n_vars][L][N], 1 <= B <= 8) of one system against one key in one
        pass over every key vector (rs_groth16_prove_batch): a tile of a host-resident or seeded key is copied / expanded once
        per batch.  pk, window as in groth16_prove (HostWords: a host key; "pub_seeds": a seeded key).  kinds: None, or one
        entry per member, each None or [n_vars] RS_KIND_*.  check: r1cs_check on every member first; ValueError naming the
        member and its first violated constraint, before anything is proved.
        Returns (proofs [B][3] encoding elements, empties [B][3]); member b's are what groth16_prove returns for it."""
        B, ptrs, keep, kp = self._batch_args(dcs, assignments, kinds, check)
        s, seeded = self._groth16_key(pk, window)
        proofs = self.enc_empty(max(B, 1), 3)
        empty = (C.c_int * (3 * max(B, 1)))()
        prove = self._prover(pk, "rs_groth16_prove_batch", "rs_groth16_prove_batch_seeded", "rs_groth16_prove_batch_packed")
        _lib.check(prove(self.h, dcs.h, C.byref(s), B, ptrs, kp, _ptr(proofs), empty, self.stream()))
        return proofs, [[int(empty[3 * b + k]) for k in range(3)] for b in range(B)]

    def rinocchio_prove_batch(self, dcs, pk, assignments, d=None, window=0, kinds=None, check=False):
        """As groth16_prove_batch (rs_rinocchio_prove_batch).  d: None (non-ZK) or a device tensor [B][3][L][N], the ring
        elements d1, d2, d3 of every member.  Returns (proofs [B][9], empties [B][9])."""
        B, ptrs, keep, kp = self._batch_args(dcs, assignments, kinds, check)
        if d is not None:
            assert self._count(d, self.ring_words) == 3 * B, "d holds d1, d2, d3 of every member"
        s, seeded = self._rinocchio_key(pk, window)
        proofs = self.enc_empty(max(B, 1), 9)
        empty = (C.c_int * (9 * max(B, 1)))()
        prove = self._prover(pk, "rs_rinocchio_prove_batch", "rs_rinocchio_prove_batch_seeded", "rs_rinocchio_prove_batch_packed")
        _lib.check(prove(self.h, dcs.h, C.byref(s), B, ptrs, kp, _ptr(d), _ptr(proofs), empty, self.stream()))
        return proofs, [[int(empty[9 * b + k]) for k in range(9)] for b in range(B)]

    def prove_batch_bytes(self, dcs, scheme, batch):
        """Bytes of context workspace a batched proof of `batch` members holds (rs_prove_batch_bytes); scheme "groth16" | "rinocchio"."""
        n = C.c_size_t(0)
        _lib.check(self.lib.rs_prove_batch_bytes(self.h, dcs.h, {"groth16": 0, "rinocchio": 1}[scheme], batch, C.byref(n)))
        return n.value

    # ---- measurement / synthetic workloads
    def set_profiling(self, on):
        _lib.check(self.lib.rs_set_profiling(self.h, 1 if on else 0))

    def last_timings(self):
        t = _lib.Timings()
        _lib.check(self.lib.rs_last_timings(self.h, C.byref(t)))
        return {k: getattr(t, k) for k, _ in _lib.Timings._fields_}

    def measure_peaks(self):
        """{hbm_copy_gbs, hbm_read_gbs, hbm_inplace_gbs, fp64_fma_T, fp64_mulmod_G, int_montmul_G} measured on this device now (rs_measure_peaks)"""
        p = _lib.Peaks()
        _lib.check(self.lib.rs_measure_peaks(self.h, C.byref(p), self.stream()))
        return {k: getattr(p, k) for k, _ in _lib.Peaks._fields_}

    def profile_read(self):
        """[{name, launches, total_ms, alg_bytes, fp64_ops}] per kernel since profiling was switched on, by time."""
        cap = 64
        arr = (_lib.KernelStat * cap)()
        n = C.c_int(0)
        _lib.check(self.lib.rs_profile_read(self.h, arr, cap, C.byref(n)))
        return [{"name": arr[k].name.decode(), "launches": arr[k].launches, "total_ms": arr[k].total_ms,
                 "alg_bytes": arr[k].alg_bytes, "fp64_ops": arr[k].fp64_ops} for k in range(min(cap, n.value))]

    def fill_uniform(self, t, layout, seed):
        words = self.ring_words if layout == 0 else self.enc_words
        _lib.check(self.lib.rs_fill_uniform(self.h, _ptr(t), self._count(t, words), layout, seed, self.stream()))
        return t

    def chain_assignment(self, assignment, m):
        _lib.check(self.lib.rs_chain_assignment(self.h, _ptr(assignment), m, self.stream()))
        return assignment
