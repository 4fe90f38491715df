/* bin_key.h -- the composite key of the common-case binning bodies (bin_fast, bin_core.hip.h; bin_select, bin_select.hip.h).
 * One definition for the kernels and for the host (pya_debug_bin_keys, host_abi.cpp), so a test can place intensities a chosen
 * number of key steps apart.
 *
 * A key is a positive float32 whose EXPONENT holds the window and whose mantissa holds the intensity:
 *     bits = (PYA_BIN_KEY_EXP0 + 63 - window) << 23 | k23
 *     k23  = (max(hw, base) - base) >> 2        hw = high word of the float64 intensity (sign 0: order-preserving)
 *     base = max hw of the spectrum - (2^25 - 1), or 0: 2^32 of dynamic range below the most intense peak (5 exponent bits),
 *            of which the key keeps the upper 23 bits (18 mantissa bits of the intensity)
 * Read as integers the keys order like (window descending, then intensity): positive float bit patterns order like integers,
 * which the second sweep (integer > / ==) and the bucket histogram of bin_select (the top six bits of k23) use.
 * Read as floats, two keys of ONE window share an exponent e >= 150: both are multiples of 2^(e - 150) >= 1, their difference is
 * exact and, when the other key is larger, at least 1: clamp(o - me) to [0, 1] is exactly 1.0 when `o` is more intense and 0.0
 * when it is not.  A key of a LATER window has a smaller exponent, so it is smaller than every key of this window: the
 * difference is negative whatever it rounds to, and clamps to 0.  The zero padding behind the last peak is 0.0f: the same.
 * (Keys of earlier windows would clamp to 1: the ranking sweep never reads them, it starts at the window's first peak.)
 * So "number of more intense mates" is a sum of clamped differences: two float instructions per mate, or two packed ones per
 * two mates, where the integer form takes subtract, shift, add. */
#ifndef PYA_BIN_KEY_H
#define PYA_BIN_KEY_H
#include <stdint.h>

#if defined(__HIPCC__)
#define PYA_BIN_KEY_HD __host__ __device__ static inline
#else
#define PYA_BIN_KEY_HD static inline
#endif

#define PYA_BIN_FAST_WINDOWS 64    /* window ids the composite key has room for */
#define PYA_BIN_KEY_BITS 23        /* intensity bits of the composite key: 5 exponent + 18 mantissa bits below the largest */
#define PYA_BIN_KEY_RANGE_BITS 25  /* bits of the high-word difference the key base leaves room for (2^32 of dynamic range) */
#define PYA_BIN_KEY_EXP0 150       /* biased exponent of the last window's keys: one ulp of such a float is 2^(150 - 127 - 23) = 1 */

static_assert(PYA_BIN_KEY_EXP0 + PYA_BIN_FAST_WINDOWS - 1 < 255, "the first window's exponent must stay finite");
static_assert(PYA_BIN_KEY_EXP0 - 127 >= PYA_BIN_KEY_BITS, "one key step must be at least 1.0 in every window");
static_assert(PYA_BIN_KEY_BITS == 23, "the intensity field is the mantissa of a float32");

/* the key base of a spectrum whose most intense peak has high word maxhw */
PYA_BIN_KEY_HD uint32_t bin_key_base(uint32_t maxhw) {
    const uint32_t range = (1u << PYA_BIN_KEY_RANGE_BITS) - 1u;
    return maxhw > range ? maxhw - range : 0u;
}
/* the intensity field: 0 for everything 2^32 or more below the most intense peak */
PYA_BIN_KEY_HD uint32_t bin_key_intensity(uint32_t hw, uint32_t base) {
    return ((hw > base ? hw : base) - base) >> (PYA_BIN_KEY_RANGE_BITS - PYA_BIN_KEY_BITS);
}
/* the key bits of a peak of window w (< PYA_BIN_FAST_WINDOWS) */
PYA_BIN_KEY_HD uint32_t bin_key_bits(uint32_t hw, uint32_t base, uint32_t w) {
    return ((uint32_t)(PYA_BIN_KEY_EXP0 + PYA_BIN_FAST_WINDOWS - 1) - w) << PYA_BIN_KEY_BITS | bin_key_intensity(hw, base);
}
/* the window back from a key */
PYA_BIN_KEY_HD uint32_t bin_key_window(uint32_t bits) {
    return (uint32_t)(PYA_BIN_KEY_EXP0 + PYA_BIN_FAST_WINDOWS - 1) - (bits >> PYA_BIN_KEY_BITS);
}

#endif
