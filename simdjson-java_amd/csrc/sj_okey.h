// sj_okey.h -- the order-preserving unsigned key of a double's bits, once for the operators that order doubles as integers:
// sj_groupstats.h (minimum and maximum per key) and sj_toprows.h (the radix select; 4.18).  IEEE totalOrder on the
// non-NaN doubles: -inf < ... < -0.0 < +0.0 < ... < +inf.  Compiles as plain C++ and as HIP device code.
#pragma once
#include <stdint.h>

#include "sj_block.h"

constexpr sj_u64 GS_INF_BITS = 0x7FF0000000000000ull, GS_SIGN = 0x8000000000000000ull;

// the order-preserving key of a double's bits and back: negative doubles have all bits flipped, the others the sign bit
SJ_HD sj_u64 gs_okey(sj_u64 bits) { return bits ^ ((bits >> 63) ? ~0ull : GS_SIGN); }
SJ_HD sj_u64 gs_okey_bits(sj_u64 key) { return key ^ ((key >> 63) ? GS_SIGN : ~0ull); }
SJ_HD bool gs_is_nan(sj_u64 bits) { return (bits & ~GS_SIGN) > GS_INF_BITS; }
