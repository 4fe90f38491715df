/* quant_rule.hip.h -- the quantum rule of the quantification stages (include/pyascore_hip.h: pya_site_quant), once: which
 * reading is usable and what integer it adds.  site_quant.hip and pform_quant.hip include it. */
#pragma once
#include "device_common.hip.h"

#define QR_SAT 281474976710656.0      /* 2^48 */

/* NaN, zeros and negatives are "no reading" */
DEV bool qr_usable(double v) { return v == v && v > 0.0; }

/* the quantum of a usable reading: v * scale (scale = 2^scale_log2, exact), 2^48 and *saturated from 2^48 on (+inf included),
 * truncated otherwise */
DEV uint64_t qr_quantum(double v, double scale, bool *saturated) {
    const double t = v * scale;
    *saturated = t >= QR_SAT;
    return *saturated ? 1ull << 48 : (uint64_t)t;
}
