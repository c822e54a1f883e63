// rc_decode_grouped_magic.hip — k_decode_static_grouped (static chunk sets, rc_chunk_set.h) for
// totals that are no power of two.
#define RC_DEC_DIV 1
#define RC_DEC_GROUPED 1
#include "rc_decode.inc"
