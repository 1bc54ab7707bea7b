"""ctypes binding of librs_hip.so (include/ringsnark_amd.h).

The library is the product: there is no CPU fallback.  Importing this module without the built
shared object raises, and every entry point raises RsError on a non-zero status.
"""
import contextlib
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "librs_hip.so")
LIB_PATH = os.environ.get("RINGSNARK_AMD_LIB", LIB_PATH)  # developer override: A/B builds of the same ABI

RS_OK, RS_ERR_INVALID, RS_ERR_HIP, RS_ERR_UNSUPPORTED, RS_ERR_NOT_INVERTIBLE, RS_ERR_NOISE = 0, 1, 2, 3, 4, 5
RS_MOD_PLAIN, RS_MOD_COEFF = 0, 1
RS_KIND_POLY, RS_KIND_ONE = 0, 2
RS_EVAL_FULL, RS_EVAL_IO, RS_EVAL_MID = 0, 1, 2
RS_SOLVE_AUTO, RS_SOLVE_LEVELS, RS_SOLVE_WALK = 0, 1, 2
RS_HINT_BITS, RS_HINT_INV, RS_HINT_QUOT = 1, 2, 3

u64p = C.POINTER(C.c_uint64)
u32p = C.POINTER(C.c_uint32)
u8p = C.POINTER(C.c_uint8)
vp = C.c_void_p


class RsError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("librs_hip error %d: %s" % (code, msg))
        self.code = code


class MsmVec(C.Structure):
    _fields_ = [("d_coeff", vp), ("h_kinds", u8p), ("T", C.c_size_t), ("group", C.c_int), ("slot_const", C.c_int)]


class Groth16PK(C.Structure):
    _fields_ = [("d_s_pows", vp), ("d_delta_ts", vp), ("d_delta_mid", vp), ("d_alpha", vp), ("d_beta", vp),
                ("window", C.c_size_t), ("host_key", C.c_int)]


class RinocchioPK(C.Structure):
    _fields_ = [("d_s_pows", vp), ("d_alpha_s_pows", vp), ("d_beta_prods", vp), ("d_beta_rv_ts", vp),
                ("d_beta_rw_ts", vp), ("d_beta_ry_ts", vp), ("window", C.c_size_t), ("host_key", C.c_int)]


class Timings(C.Structure):
    _fields_ = [("evaluate_ms", C.c_float), ("witness_ms", C.c_float), ("msm_ms", C.c_float), ("total_ms", C.c_float)]


class Peaks(C.Structure):
    _fields_ = [("hbm_copy_gbs", C.c_double), ("fp64_fma_T", C.c_double), ("fp64_mulmod_G", C.c_double), ("int_montmul_G", C.c_double),
                ("hbm_read_gbs", C.c_double), ("hbm_inplace_gbs", C.c_double)]


class R1csReport(C.Structure):
    _fields_ = [("n_violated", C.c_uint64), ("first_row", C.c_uint64), ("first_limb", C.c_uint32), ("first_slot", C.c_uint32),
                ("a", C.c_uint64), ("b", C.c_uint64), ("c", C.c_uint64)]


class SolveInfo(C.Structure):
    _fields_ = [("n_given", C.c_uint64), ("n_solved", C.c_uint64), ("n_unsolved", C.c_uint64), ("first_unsolved", C.c_uint64),
                ("n_levels", C.c_uint64), ("max_width", C.c_uint64), ("n_unused", C.c_uint64), ("first_blocked", C.c_uint64),
                ("blocked_reason", C.c_uint32)]


class SolveStats(C.Structure):
    _fields_ = [("level_launches", C.c_uint32), ("walk_launches", C.c_uint32)]


class SolveHint(C.Structure):  # rs_solve_hint: 0-based variables
    _fields_ = [("kind", C.c_uint32), ("src", C.c_uint32), ("num", C.c_uint32), ("dst", C.c_uint32), ("nbits", C.c_uint32),
                ("dst_stride", C.c_uint32)]


class HintInfo(C.Structure):
    _fields_ = [("solve", SolveInfo), ("n_steps", C.c_uint64), ("n_hints_run", C.c_uint64), ("n_hints_blocked", C.c_uint64),
                ("first_blocked_hint", C.c_uint64)]


class HintStats(C.Structure):
    _fields_ = [("level_launches", C.c_uint32), ("walk_launches", C.c_uint32), ("hint_launches", C.c_uint32)]


class HintReport(C.Structure):
    _fields_ = [("n_bits_bad", C.c_uint64), ("bad_hint", C.c_uint32), ("bad_limb", C.c_uint32), ("bad_slot", C.c_uint32),
                ("reserved0", C.c_uint32), ("n_zero", C.c_uint64), ("zero_hint", C.c_uint32), ("zero_limb", C.c_uint32),
                ("zero_slot", C.c_uint32), ("reserved1", C.c_uint32)]


class VerifyReport(C.Structure):
    _fields_ = [("accepted", C.c_uint32), ("failed", C.c_uint32), ("n_bad", C.c_uint64 * 6), ("first_check", C.c_uint32),
                ("first_limb", C.c_uint32), ("first_slot", C.c_uint32), ("lhs", C.c_uint64), ("rhs", C.c_uint64)]


class InvReport(C.Structure):
    _fields_ = [("n_zero", C.c_uint64), ("zero_elem", C.c_uint64), ("zero_limb", C.c_uint32), ("zero_slot", C.c_uint32),
                ("n_bad", C.c_uint64), ("bad_elem", C.c_uint64), ("bad_limb", C.c_uint32), ("bad_slot", C.c_uint32),
                ("bad_x", C.c_uint64), ("bad_num", C.c_uint64)]


class BitsReport(C.Structure):
    _fields_ = [("n_bad", C.c_uint64), ("first_elem", C.c_uint64), ("first_limb", C.c_uint32), ("first_slot", C.c_uint32),
                ("word", C.c_uint64), ("value", C.c_uint64)]


class Groth16KeyOut(C.Structure):
    _fields_ = [("s_pows", vp), ("delta_ts", vp), ("delta_mid", vp), ("d_alpha", vp), ("d_beta", vp), ("host_key", C.c_int),
                ("tile", C.c_size_t)]


class RinocchioKeyOut(C.Structure):
    _fields_ = [("s_pows", vp), ("alpha_s_pows", vp), ("beta_prods", vp), ("d_beta_rv_ts", vp), ("d_beta_rw_ts", vp),
                ("d_beta_ry_ts", vp), ("host_key", C.c_int), ("tile", C.c_size_t)]


class Groth16SeededKeyOut(Groth16KeyOut):  # rs_groth16_seeded_key_out: the same members, the three vectors compact
    pass


class RinocchioSeededKeyOut(RinocchioKeyOut):
    pass


class Groth16PKSeeded(C.Structure):
    _fields_ = [("s_pows", vp), ("delta_ts", vp), ("delta_mid", vp), ("pub_seeds", C.c_uint64 * 3), ("d_alpha", vp), ("d_beta", vp),
                ("window", C.c_size_t), ("host_key", C.c_int)]


class RinocchioPKSeeded(C.Structure):
    _fields_ = [("s_pows", vp), ("alpha_s_pows", vp), ("beta_prods", vp), ("pub_seeds", C.c_uint64 * 3), ("d_beta_rv_ts", vp),
                ("d_beta_rw_ts", vp), ("d_beta_ry_ts", vp), ("window", C.c_size_t), ("host_key", C.c_int)]


class KernelStat(C.Structure):
    _fields_ = [("name", C.c_char * 48), ("launches", C.c_int), ("total_ms", C.c_float), ("alg_bytes", C.c_double),
                ("fp64_ops", C.c_double)]


# name -> (restype, argtypes); every function of include/ringsnark_amd.h
SIGNATURES = {
    "rs_last_error": (C.c_char_p, []),
    "rs_version": (C.c_int, []),
    "rs_ctx_create": (C.c_int, [C.c_int, C.c_int, C.c_int, u64p, C.c_int, C.c_int, u64p, C.POINTER(vp)]),
    "rs_ctx_destroy": (None, [vp]),
    "rs_malloc": (C.c_int, [vp, C.c_size_t, C.POINTER(vp)]),
    "rs_free": (C.c_int, [vp, vp]),
    "rs_upload": (C.c_int, [vp, vp, vp, C.c_size_t, vp]),
    "rs_download": (C.c_int, [vp, vp, vp, C.c_size_t, vp]),
    "rs_sync": (C.c_int, [vp, vp]),
    "rs_ntt_forward": (C.c_int, [vp, C.c_int, C.c_int, vp, C.c_size_t, vp]),
    "rs_ntt_inverse": (C.c_int, [vp, C.c_int, C.c_int, vp, C.c_size_t, vp]),
    "rs_ring_add": (C.c_int, [vp, vp, vp, vp, C.c_size_t, vp]),
    "rs_ring_sub": (C.c_int, [vp, vp, vp, vp, C.c_size_t, vp]),
    "rs_ring_mul": (C.c_int, [vp, vp, vp, vp, C.c_size_t, vp]),
    "rs_ring_neg": (C.c_int, [vp, vp, vp, C.c_size_t, vp]),
    "rs_ring_add_scalar": (C.c_int, [vp, vp, vp, C.c_uint64, C.c_size_t, vp]),
    "rs_ring_mul_scalar": (C.c_int, [vp, vp, vp, C.c_uint64, C.c_size_t, vp]),
    "rs_ring_inv": (C.c_int, [vp, vp, vp, C.c_size_t, vp]),
    "rs_ring_is_zero": (C.c_int, [vp, vp, C.c_size_t, u8p, vp]),
    "rs_batch_encode": (C.c_int, [vp, vp, vp, C.c_size_t, vp]),
    "rs_enc_mul_ring": (C.c_int, [vp, vp, vp, C.c_size_t, vp]),
    "rs_enc_add": (C.c_int, [vp, vp, vp, vp, C.c_size_t, vp]),
    "rs_enc_reduce": (C.c_int, [vp, vp, C.c_size_t, vp]),
    "rs_enc_wire_size": (C.c_size_t, [vp, C.c_size_t]),
    "rs_enc_serialize": (C.c_int, [vp, vp, u8p, C.c_size_t, vp, C.c_size_t, vp]),
    "rs_enc_deserialize": (C.c_int, [vp, vp, C.c_size_t, vp, u8p, C.c_size_t, C.POINTER(C.c_size_t), vp]),
    "rs_instance_map_eval": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    "rs_enc_decode": (C.c_int, [vp, vp, vp, C.c_size_t, vp, vp]),
    "rs_enc_noise_budget": (C.c_int, [vp, vp, vp, C.c_size_t, C.POINTER(C.c_int), vp]),
    "rs_enc_encode": (C.c_int, [vp, vp, vp, C.c_size_t, C.c_uint64, vp, vp]),
    "rs_inner_product": (C.c_int, [vp, vp, vp, u8p, C.c_size_t, vp, C.POINTER(C.c_size_t), vp]),
    "rs_msm": (C.c_int, [vp, C.POINTER(vp), C.c_int, C.c_size_t, C.c_size_t, C.POINTER(MsmVec), C.c_int, C.c_int, vp,
                         C.POINTER(C.c_size_t), vp]),
    "rs_msm_hostkey": (C.c_int, [vp, C.POINTER(vp), C.c_int, C.c_size_t, C.c_size_t, C.POINTER(MsmVec), C.c_int, C.c_int, vp,
                                 C.POINTER(C.c_size_t), vp]),
    "rs_host_alloc": (C.c_int, [vp, C.c_size_t, C.POINTER(vp)]),
    "rs_host_free": (C.c_int, [vp, vp]),
    "rs_r1cs_create": (C.c_int, [vp, C.c_size_t, C.c_size_t, C.c_size_t, C.POINTER(u32p), C.POINTER(u32p),
                                 C.POINTER(u64p), C.POINTER(C.c_size_t), C.POINTER(vp)]),
    "rs_r1cs_create_poly": (C.c_int, [vp, C.c_size_t, C.c_size_t, C.c_size_t, C.POINTER(u32p), C.POINTER(u32p),
                                      C.POINTER(u64p), C.POINTER(C.c_size_t), C.POINTER(C.POINTER(C.c_int32)), u64p, C.c_size_t,
                                      C.POINTER(vp)]),
    "rs_r1cs_destroy": (None, [vp]),
    "rs_r1cs_evaluate": (C.c_int, [vp, vp, C.c_int, C.c_int, vp, vp, vp]),
    "rs_witness_map": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, u64p, vp]),
    "rs_witness_map_slots": (C.c_int, [vp, vp, vp, vp, vp, vp, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp, u64p, vp]),
    "rs_witness_map_rows": (C.c_int, [vp, vp, vp, vp, vp, vp, C.POINTER(C.c_size_t), vp, vp, vp, vp, vp, vp, vp, u64p, vp]),
    "rs_interpolate": (C.c_int, [vp, vp, vp, C.c_size_t, vp]),
    "rs_poly_multiply": (C.c_int, [vp, vp, C.c_size_t, vp, C.c_size_t, vp, C.POINTER(C.c_size_t), vp]),
    "rs_poly_add": (C.c_int, [vp, vp, C.c_size_t, vp, C.c_size_t, vp, C.POINTER(C.c_size_t), vp]),
    "rs_poly_divide": (C.c_int, [vp, vp, C.c_size_t, vp, C.c_size_t, vp, C.POINTER(C.c_size_t), vp]),
    "rs_groth16_prove": (C.c_int, [vp, vp, C.POINTER(Groth16PK), vp, vp, C.POINTER(C.c_int), vp]),
    "rs_rinocchio_prove": (C.c_int, [vp, vp, C.POINTER(RinocchioPK), vp, vp, vp, vp, vp, C.POINTER(C.c_int), vp]),
    "rs_groth16_prove_kinds": (C.c_int, [vp, vp, C.POINTER(Groth16PK), vp, u8p, vp, C.POINTER(C.c_int), vp]),
    "rs_rinocchio_prove_kinds": (C.c_int, [vp, vp, C.POINTER(RinocchioPK), vp, u8p, vp, vp, vp, vp, C.POINTER(C.c_int), vp]),
    "rs_last_timings": (C.c_int, [vp, C.POINTER(Timings)]),
    "rs_measure_peaks": (C.c_int, [vp, C.POINTER(Peaks), vp]),
    "rs_set_profiling": (C.c_int, [vp, C.c_int]),
    "rs_profile_read": (C.c_int, [vp, C.POINTER(KernelStat), C.c_int, C.POINTER(C.c_int)]),
    "rs_set_tuning": (C.c_int, [C.c_char_p, C.c_int]),
    "rs_fill_uniform": (C.c_int, [vp, vp, C.c_size_t, C.c_int, C.c_uint64, vp]),
    "rs_chain_assignment": (C.c_int, [vp, vp, C.c_size_t, vp]),
}

TUNING_SIGNATURES = {  # every function of include/ringsnark_amd/tuning.h
    "rs_get_tuning": (C.c_int, [C.c_char_p, C.POINTER(C.c_int)]),
    "rs_tuning_key": (C.c_char_p, [C.c_int]),
}

CHECK_SIGNATURES = {  # every function of include/ringsnark_amd/r1cs_check.h
    "rs_r1cs_check": (C.c_int, [vp, vp, vp, vp, C.POINTER(R1csReport), vp]),
}

SOLVE_SIGNATURES = {  # every function of include/ringsnark_amd/r1cs_solve.h
    "rs_r1cs_solve_plan_create": (C.c_int, [vp, vp, u8p, C.POINTER(vp), C.POINTER(SolveInfo)]),
    "rs_r1cs_solve_plan_steps": (C.c_int, [vp, u32p, u32p, u64p]),
    "rs_r1cs_solve_plan_destroy": (None, [vp]),
    "rs_r1cs_solve": (C.c_int, [vp, vp, vp, C.c_int, C.POINTER(SolveStats), vp]),
}

HINT_SIGNATURES = {  # every function of include/ringsnark_amd/solve_hints.h
    "rs_r1cs_hint_plan_create": (C.c_int, [vp, vp, u8p, C.POINTER(SolveHint), C.c_size_t, C.POINTER(vp), C.POINTER(HintInfo)]),
    "rs_r1cs_hint_plan_steps": (C.c_int, [vp, u8p, u32p, u32p, u64p]),
    "rs_r1cs_hint_plan_destroy": (None, [vp]),
    "rs_r1cs_solve_hinted": (C.c_int, [vp, vp, vp, C.c_int, C.POINTER(HintStats), C.POINTER(HintReport), vp]),
}

VERIFY_SIGNATURES = {  # every function of include/ringsnark_amd/verify.h
    "rs_io_eval_at": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, vp]),
    "rs_groth16_vk_create": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, vp, C.POINTER(vp)]),
    "rs_groth16_vk_destroy": (None, [vp]),
    "rs_rinocchio_vk_create": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, vp, vp, C.POINTER(vp)]),
    "rs_rinocchio_vk_destroy": (None, [vp]),
    "rs_groth16_verify": (C.c_int, [vp, vp, vp, vp, C.POINTER(C.c_int), C.POINTER(VerifyReport), vp]),
    "rs_rinocchio_verify": (C.c_int, [vp, vp, vp, vp, C.POINTER(C.c_int), C.POINTER(VerifyReport), vp]),
}

KEYGEN_SIGNATURES = {  # every function of include/ringsnark_amd/keygen.h
    "rs_groth16_keygen": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, u64p, C.POINTER(Groth16KeyOut), vp]),
    "rs_rinocchio_keygen": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, vp, vp, u64p, C.POINTER(RinocchioKeyOut), vp]),
    "rs_enc_encode_linear": (C.c_int, [vp, vp, C.POINTER(vp), C.POINTER(vp), C.c_int, C.c_size_t, C.c_uint64, vp, vp]),
}

SEEDED_SIGNATURES = {  # every function of include/ringsnark_amd/seeded.h
    "rs_enc_expand_seeded": (C.c_int, [vp, vp, C.c_uint64, C.c_size_t, C.c_size_t, vp, vp]),
    "rs_groth16_keygen_seeded": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, u64p, u64p, C.POINTER(Groth16SeededKeyOut), vp]),
    "rs_rinocchio_keygen_seeded": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, vp, vp, u64p, u64p, C.POINTER(RinocchioSeededKeyOut), vp]),
    "rs_msm_seeded": (C.c_int, [vp, C.POINTER(vp), u64p, C.c_int, C.c_int, C.c_size_t, C.c_size_t, C.POINTER(MsmVec), C.c_int, C.c_int, vp,
                                C.POINTER(C.c_size_t), vp]),
    "rs_groth16_prove_seeded": (C.c_int, [vp, vp, C.POINTER(Groth16PKSeeded), vp, u8p, vp, C.POINTER(C.c_int), vp]),
    "rs_rinocchio_prove_seeded": (C.c_int, [vp, vp, C.POINTER(RinocchioPKSeeded), vp, u8p, vp, vp, vp, vp, C.POINTER(C.c_int), vp]),
}

BATCH_SIGNATURES = {  # every function of include/ringsnark_amd/batch.h
    "rs_groth16_prove_batch": (C.c_int, [vp, vp, C.POINTER(Groth16PK), C.c_int, C.POINTER(vp), u8p, vp, C.POINTER(C.c_int), vp]),
    "rs_rinocchio_prove_batch": (C.c_int, [vp, vp, C.POINTER(RinocchioPK), C.c_int, C.POINTER(vp), u8p, vp, vp, C.POINTER(C.c_int), vp]),
    "rs_groth16_prove_batch_seeded": (C.c_int, [vp, vp, C.POINTER(Groth16PKSeeded), C.c_int, C.POINTER(vp), u8p, vp, C.POINTER(C.c_int), vp]),
    "rs_rinocchio_prove_batch_seeded": (C.c_int, [vp, vp, C.POINTER(RinocchioPKSeeded), C.c_int, C.POINTER(vp), u8p, vp, vp,
                                                  C.POINTER(C.c_int), vp]),
    "rs_prove_batch_bytes": (C.c_int, [vp, vp, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
}

MODSWITCH_SIGNATURES = {  # every function of include/ringsnark_amd/modswitch.h
    "rs_enc_mod_switch": (C.c_int, [vp, vp, C.c_size_t, C.c_int, C.c_int, vp, vp]),
    "rs_enc_decode_level": (C.c_int, [vp, C.c_int, vp, vp, C.c_size_t, vp, vp]),
    "rs_enc_noise_budget_level": (C.c_int, [vp, C.c_int, vp, vp, C.c_size_t, C.POINTER(C.c_int), vp]),
    "rs_enc_wire_size_level": (C.c_size_t, [vp, C.c_int, C.c_size_t]),
    "rs_enc_serialize_level": (C.c_int, [vp, C.c_int, vp, u8p, C.c_size_t, vp, C.c_size_t, vp]),
    "rs_enc_deserialize_level": (C.c_int, [vp, vp, C.c_size_t, vp, u8p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_int), vp]),
    "rs_groth16_verify_level": (C.c_int, [vp, vp, C.c_int, vp, vp, C.POINTER(C.c_int), C.POINTER(VerifyReport), vp]),
    "rs_rinocchio_verify_level": (C.c_int, [vp, vp, C.c_int, vp, vp, C.POINTER(C.c_int), C.POINTER(VerifyReport), vp]),
}

BITS_SIGNATURES = {  # every function of include/ringsnark_amd/bits.h
    "rs_ring_bit_decompose": (C.c_int, [vp, vp, C.c_size_t, C.c_size_t, C.c_int, vp, C.c_size_t, C.POINTER(BitsReport), vp]),
}

INVERSE_SIGNATURES = {  # every function of include/ringsnark_amd/inverse.h
    "rs_ring_inv_or_zero": (C.c_int, [vp, vp, C.c_size_t, vp, C.c_size_t, C.c_size_t, vp, C.c_size_t, C.POINTER(InvReport), vp]),
}

VERIFY_BATCH_SIGNATURES = {  # every function of include/ringsnark_amd/verify_batch.h
    "rs_verify_batch_group": (C.c_int, []),
    "rs_groth16_verify_batch": (C.c_int, [vp, vp, C.c_int, C.c_int, vp, vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                          C.POINTER(VerifyReport), vp]),
    "rs_rinocchio_verify_batch": (C.c_int, [vp, vp, C.c_int, C.c_int, vp, vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                            C.POINTER(VerifyReport), vp]),
}
R1CS_BATCH_SIGNATURES = {  # every function of include/ringsnark_amd/r1cs_batch.h
    "rs_r1cs_solve_batch": (C.c_int, [vp, vp, C.c_int, C.POINTER(vp), C.c_int, C.POINTER(SolveStats), vp]),
    "rs_r1cs_check_batch": (C.c_int, [vp, vp, C.c_int, C.POINTER(vp), vp, C.POINTER(R1csReport), vp]),
}
PACKED_SIGNATURES = {  # every function of include/ringsnark_amd/packed.h
    "rs_enc_pack_bits": (C.c_int, [vp]),
    "rs_enc_packed_words": (C.c_size_t, [vp]),
    "rs_enc_pack_c0": (C.c_int, [vp, vp, C.c_size_t, vp, C.POINTER(C.c_size_t), vp]),
    "rs_enc_unpack_c0": (C.c_int, [vp, vp, C.c_size_t, vp, vp]),
    "rs_enc_expand_packed": SEEDED_SIGNATURES["rs_enc_expand_seeded"],
    "rs_groth16_keygen_packed": SEEDED_SIGNATURES["rs_groth16_keygen_seeded"],
    "rs_rinocchio_keygen_packed": SEEDED_SIGNATURES["rs_rinocchio_keygen_seeded"],
    "rs_msm_packed": SEEDED_SIGNATURES["rs_msm_seeded"],
    "rs_groth16_prove_packed": SEEDED_SIGNATURES["rs_groth16_prove_seeded"],
    "rs_rinocchio_prove_packed": SEEDED_SIGNATURES["rs_rinocchio_prove_seeded"],
    "rs_groth16_prove_batch_packed": BATCH_SIGNATURES["rs_groth16_prove_batch_seeded"],
    "rs_rinocchio_prove_batch_packed": BATCH_SIGNATURES["rs_rinocchio_prove_batch_seeded"],
}
VERIFY_BATCH_MAX = 64  # RS_VERIFY_BATCH_MAX
VERIFY_BATCH_GROUP = 4  # rs_verify_batch_group(): proofs whose public sums one thread of the check kernel carries (csrc/verify.hip VERIFY_PB)

_lib = None


def load():
    """dlopen librs_hip.so and bind every declared symbol.  Raises if the library is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "ringsnark_amd/librs_hip.so is not built (run `python -c 'import __graft_entry__ as g; g.build()'`); "
            "the HIP library is the only implementation, there is no CPU fallback")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in {**SIGNATURES, **TUNING_SIGNATURES, **CHECK_SIGNATURES, **SOLVE_SIGNATURES, **VERIFY_SIGNATURES,
                              **KEYGEN_SIGNATURES, **SEEDED_SIGNATURES, **BATCH_SIGNATURES, **MODSWITCH_SIGNATURES, **BITS_SIGNATURES,
                              **VERIFY_BATCH_SIGNATURES, **PACKED_SIGNATURES, **R1CS_BATCH_SIGNATURES,
                              **INVERSE_SIGNATURES, **HINT_SIGNATURES}.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(status):
    if status != RS_OK:
        raise RsError(status, load().rs_last_error().decode("utf-8", "replace"))


# ---- tuning knobs (csrc/tuning.hpp): process-wide, every accepted value gives identical results ----
def set_tuning(key, value):
    check(load().rs_set_tuning(key.encode(), int(value)))


def get_tuning(key):
    v = C.c_int()
    check(load().rs_get_tuning(key.encode(), C.byref(v)))
    return v.value


def tuning_keys():
    keys = []
    while (k := load().rs_tuning_key(len(keys))) is not None:
        keys.append(k.decode())
    return keys


@contextlib.contextmanager
def tuning(**knobs):
    """Scoped override: sets the named knobs in argument order and, on exit (normal or not), writes the values they had
    back in reverse order.  If a set raises, the knobs set before it are restored before the error propagates."""
    with contextlib.ExitStack() as stack:
        for key, value in knobs.items():
            saved = get_tuning(key)
            set_tuning(key, value)
            stack.callback(set_tuning, key, saved)
        yield


def tuning_from_env(name="RS_TUNING"):
    """Sets the knobs listed as `key=value,key=value` in the environment variable `name` (developer tools).
    Empty entries are skipped; an entry without `=` or with an unknown key raises."""
    for kv in filter(None, os.environ.get(name, "").split(",")):
        set_tuning(*kv.split("="))


def source_hash():
    """sha256 (first 16 hex digits) over the sources the device library is built from: ringsnark_amd/csrc/*.{hip,hpp},
    csrc/Makefile, include/ringsnark_amd.h, include/ringsnark_amd/tuning.h and include/ringsnark_amd/r1cs_check.h.  profiles/*_pmc_*.json carry it, so that bench.py can tell whether a
    committed counter file was collected on the kernels it is running (round-3 verdict: nothing tied the two)."""
    import glob
    import hashlib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    files = sorted(glob.glob(os.path.join(root, "ringsnark_amd", "csrc", "*.hip")) + glob.glob(os.path.join(root, "ringsnark_amd", "csrc", "*.hpp")))
    files += [os.path.join(root, "ringsnark_amd", "csrc", "Makefile"), os.path.join(root, "include", "ringsnark_amd.h"),
              os.path.join(root, "include", "ringsnark_amd", "tuning.h"), os.path.join(root, "include", "ringsnark_amd", "r1cs_check.h")]
    h = hashlib.sha256()
    for f in files:
        h.update(os.path.basename(f).encode())
        h.update(open(f, "rb").read())
    return h.hexdigest()[:16]
