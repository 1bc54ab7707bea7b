/* ringsnark_amd/tuning.h -- reading the kernel-shape knobs that rs_set_tuning of ringsnark_amd.h writes.  Process-wide (neither
 * per-context nor thread-safe), read by the next launch / plan build / context creation; identical results for every accepted
 * value.  Names, defaults, accepted values and meanings are ONE table, ringsnark_amd/csrc/tuning.hpp: the list in the comment
 * above rs_set_tuning is a historical excerpt of it (ringsnark_amd.h is pinned by checksum to the build of oracle/_ref that
 * compiled it against the reference's templates, tests/test_cabi.py, and changes only with the ABI the adapters use). */
#ifndef RINGSNARK_AMD_TUNING_H
#define RINGSNARK_AMD_TUNING_H
#ifdef __cplusplus
extern "C" {
#endif
int rs_get_tuning(const char *key, int *value); /* the stored (normalised) value; unknown key: RS_ERR_INVALID */
const char *rs_tuning_key(int index);           /* the knob names in table order; NULL past the end */
#ifdef __cplusplus
}
#endif
#endif
