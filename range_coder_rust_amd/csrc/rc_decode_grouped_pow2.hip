// rc_decode_grouped_pow2.hip — k_decode_static_grouped (static chunk sets, rc_chunk_set.h) for
// power-of-two totals.
#define RC_DEC_DIV 0
#define RC_DEC_GROUPED 1
#include "rc_decode.inc"
