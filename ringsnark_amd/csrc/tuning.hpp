// tuning.hpp -- the kernel-shape knobs of librs_hip.so: THE place where a knob's name, default, validation and meaning are
// written.  struct Tuning, the table behind rs_set_tuning / rs_get_tuning / rs_tuning_key (rs_core.hip) and every list of
// knobs outside the library derive from the rows below.  Contract: one process-wide instance (rs::g_tune), host variables
// only; a set takes effect at the next launch / plan build / context creation; every accepted value gives identical results
// (the result-altering ntt_repeat is settable under -DRS_EXPERIMENTS only).  Neither per-context nor thread-safe:
// tests and tools/ flip knobs between calls, from one thread; the product never changes one.
//
// Row: X(name, default, rule, lo, hi, reject, meaning); lo, hi and reject (the message of a rejection, after the name) matter
// to RANGE only.  Rules (rs::TuneRule) -- ANY: stored as given; BOOL: stored value ? 1 : 0; MIN1: stored max(1, value);
// RANGE: outside [lo, hi] rejected (RS_ERR_INVALID); FORCE_BC: 0 or 5..20 (tune_check_force_bc, rs_core.hip); SUB_CT: 0 or 2,
// others RS_ERR_UNSUPPORTED (tune_check_sub_ct, rs_core.hip).
#pragma once
#include <climits>

#define RS_TUNING_KNOBS(X)                                                                                                        \
  X(ntt_variant, 14, ANY, 0, 0, "", "negacyclic transform kernel, see launch_ntt -- 14: wide kernels of ntt_wide.hpp at 2^12..2^14, else as 8; 8..13: wave-private kernel where the length allows, else as 0; others: barrier kernel") \
  X(force_int_arith, 0, BOOL, 0, 0, "", "contexts created from now on use Montgomery integers whatever the prime sizes (tests)")      \
  X(mac_variant, 5, ANY, 0, 0, "", ">= 5: wide kernels at N_enc = 8192 and 16384 (mac_kernel_v3 / mac_kernel_v4), else as 4; 2..4: 512-thread streaming kernel at N_enc = 2048..8192 (mac_kernel_v2; 2: generic kernel for two key vectors); <= 1: generic kernel") \
  X(mac_ct_temporal, 0, BOOL, 0, 0, "", "mac_kernel_v3 reads the ciphertext words with temporal loads (A/B of L2 hits on a shared key)") \
  X(plain_variant, 1, ANY, 0, 0, "", "1: plain_center_wide_kernel at N_enc = 8192; 0: plain_center_kernel")                           \
  X(prover_lin_io, 1, ANY, 0, 0, "", "io vectors of groth16::prover as linear forms (MsmLin)")                                        \
  X(msm_host_tile, 1024, MIN1, 0, 0, "", "terms per staging buffer of a host-resident key")                                           \
  X(msm_c_mib, 2048, RANGE, 1, INT_MAX, "must be positive", "workspace of the centred plaintext rows of one term tile")                               \
  X(mac_chunk_units, 768, MIN1, 0, 0, "", "(limb, prime, chunk) units per MAC launch (term chunks = units / (L K))")                  \
  X(mac_share_keys, 1, BOOL, 0, 0, "", "two key vectors share the plaintext spectrum (mac_kernel_v4; 8192 and 16384 points)")         \
  X(ntt_wide_grid, 256, MIN1, 0, 0, "", "ntt_wide.hpp kernels: CUs to fill (workgroups = this x what fits one CU)")                   \
  X(int_ntt_variant, 1, ANY, 0, 0, "", "1: ntt_io_kernel (lengths >= 2^10); 0: ntt_generic_kernel")                                   \
  X(witness_sub_log, 12, RANGE, 12, 13, "must be 12 or 13", "12: rooted sub-transforms on blocks of 2^12 (sub_ntt_w12_kernel) where sub_block_log says so; 13: never") \
  X(witness_h_coset, 1, BOOL, 0, 0, "", "H on a coset (four length-M transforms) when the call interpolates C; 0: always big_h")      \
  X(witness_sub12_cross, 4, RANGE, 1, 8, "must be in [1, 8]", "most cross stages of a transform that takes 2^12 blocks")                               \
  X(witness_cross_pair, 1, BOOL, 0, 0, "", "two groups per thread and 16-byte accesses in the cross passes (0: the round-3 form)")    \
  X(witness_cross_maxr, 6, RANGE, 1, 6, "must be in [1, 6]", "most stages of one cross pass (FP64 arithmetic; 4: the round-3 passes)")                 \
  X(witness_force_bc, 0, FORCE_BC, 0, 0, "", "pretend the ring primes have only this 2-adicity (tests: the block paths); plans built afterwards") \
  X(witness_bc2, 1, BOOL, 0, 0, "", "two-dimensional block convolutions where they apply (0: the pairwise form); plans built afterwards") \
  X(witness_inc, 1, BOOL, 0, 0, "", "ring primes without a 2M-th root of unity run INCOMPLETE transforms (witness_inc.hpp) where build_plan's conditions hold; 0: block convolutions; plans built afterwards")                  \
  X(witness_tree_log, 14, RANGE, 13, 14, "must be 13 or 14", "largest tile (log2) of the wide product-tree kernel")                                   \
  X(witness_sub_ct, 2, SUB_CT, 0, 0, "", "2^13 sub-transforms of the multi-pass path -- 2: sub_ntt_wide_kernel; 0: generic kernel; 1 and 3 (retired kernels): RS_ERR_UNSUPPORTED")  \
  X(witness_tree_ct, 2, ANY, 0, 0, "", "2: wide product-tree kernel (tree_wide_kernel); 1: level-unrolled tree_columns_kernel; 0: level loop") \
  X(witness_tree_fwd, 0, BOOL, 0, 0, "", "the 2^14 tile kernel runs the forward cross stages of level 15 (off: measured slower, see tree_fwd_ok)") \
  X(witness_level_turn, 1, BOOL, 0, 0, "", "fuse the last inverse cross pass of tree level l with the first forward pass of level l + 1") \
  X(witness_h_turn, 1, BOOL, 0, 0, "", "fuse the last inverse cross pass of A B with the first forward pass of rev(A B)")             \
  X(witness_tree_once, 1, BOOL, 0, 0, "", "the product tree's tiles in one launch per chunk of columns")                              \
  X(witness_big_ws_mib, 6144, RANGE, 64, INT_MAX, "must be at least 64", "the two [cols][2M] workspaces of a multi-pass sub-chunk of columns")           \
  X(witness_col_budget_mib, 16384, RANGE, 1, INT_MAX, "must be positive", "column workspace of one chunk of the witness map")                         \
  X(witness_lds_logM, 13, RANGE, 6, 13, "must be in [6, 13]", "largest column (log2) that runs entirely inside one LDS tile")
// This one CHANGES THE RESULTS (timing experiments of tools/): a member always, a key of the table under RS_EXPERIMENTS only.
#define RS_TUNING_KNOBS_EXPERIMENTS(X) \
  X(ntt_repeat, 1, ANY, 0, 0, "", "wave-private transform kernel: low 8 bits = runs of the transform on its LDS tile, bits 8.. = stagger_start units")

namespace rs {
enum class TuneRule { ANY, BOOL, MIN1, RANGE, FORCE_BC, SUB_CT };
struct Tuning {
#define RS_TUNING_MEMBER(name, def, rule, lo, hi, reject, doc) int name = def;
  RS_TUNING_KNOBS(RS_TUNING_MEMBER)
  RS_TUNING_KNOBS_EXPERIMENTS(RS_TUNING_MEMBER)
#undef RS_TUNING_MEMBER
};
extern Tuning g_tune;  // rs_core.hip
}  // namespace rs
