/* bin_spectra.hip -- kernel 1: raw peaks -> retained-peak table (one spectrum per wavefront).
 *
 * Replaces BinnedSpectra::consumeSpectra + sortTopSpectra (cpp/Spectra.cpp:43-68, :24-41) and
 * the (bin, rank) peak feed of Ascore.pyx:142-150.  Output per spectrum: the retained peaks
 * (the n_top = 10 most intense of every bin_size-wide window) as float32 m/z in ascending
 * order plus their intensity rank inside their window -- exactly the information the match
 * cache of the reference holds (ModifiedPeptide.cpp:126-142).
 *
 * HBM traffic: reads 16 B per raw peak once (coalesced, 8 B per lane), writes 8 B per retained
 * peak.  Everything else lives in LDS (bin_core.hip.h).  Typed spectra (pya_plan_run_typed): every kernel
 * of the family exists for <double, double>, <double, float> and <float, float> m/z and intensity arrays
 * (12 and 8 B per raw peak); a value is widened where it is loaded, so the three compute the same table
 * from arrays that hold the same values, and a hand-over list is worked off by the same types.
 *
 * Two kernels: pya_bin_spectra_kernel takes the common case (peaks in m/z order, no two equal
 * intensities inside a window) and appends every other spectrum to a list that
 * pya_bin_exact_kernel works off -- any peak order, ties resolved as std::nth_element + std::sort
 * resolve them.  The rare paths stay out of the hot kernel's register budget that way.
 */
#include "bin_core.hip.h"
#include "bin_select.hip.h"

#ifndef BIN_WAVES
#define BIN_WAVES 4     /* independent spectra per workgroup when LDS allows (no cross-wave sync) */
#endif

template <typename MZ, typename IT>
__global__ __launch_bounds__(64 * BIN_WAVES) void pya_bin_spectra_kernel(BatchDev b, const uint32_t *psm_ids,
                                                                         uint32_t n_ids, uint32_t cap) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_all[];
    /* (the wavefront's number as a scalar: the spectrum's offsets, length and pointers then live in scalar registers and
     * the tests on them are scalar branches) */
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t slot = xcd_slot(blockIdx.x, gridDim.x) * (blockDim.x >> 6) + wave;
    /* the plan's runs alternate between two sets of hand-over counts: this run zeroes the next one's (nothing of this
     * run touches them, everything of the run before has finished) -- no memset between the runs */
    if (blockIdx.x == 0 && threadIdx.x < 3 && b.zero_next) b.zero_next[threadIdx.x] = 0u;
    if (slot >= n_ids) return;
    unsigned char *lds_raw = lds_all + (size_t)wave * PYA_BIN_FAST_BYTES(cap);
    const uint32_t psm = psm_ids[slot];
    const float *r_mz;
    const uint8_t *r_rank;
    int status;
    const int R = bin_fast<true, false, MZ, IT>(b, psm, lds_raw, cap, &r_mz, &r_rank, &status);   /* (stores the table itself) */
    if (R == PYA_BIN_REDO) {
        /* peaks out of m/z order or equal intensities in a window: left to pya_bin_exact_kernel */
        if (lane_id() == 0) b.redo_ids[atomicAdd(b.redo_count, 1u)] = psm;
        return;
    }
    if (R < 0) bin_store(b, psm, R, status, r_mz, r_rank);                        /* (no windows: the status only) */
}

/* Dense spectra (the host sends the peak classes above pya_handle.kn.bin_select_min here): selection by per-window
 * histograms, then bin_fast's ranking over the survivors only (bin_select.hip.h) -- O(peaks), LDS independent of the peak
 * count.  What it declines goes to the same list. */
template <typename MZ, typename IT>
__global__ __launch_bounds__(64 * BIN_WAVES) void pya_bin_select_kernel(BatchDev b, const uint32_t *psm_ids, uint32_t n_ids,
                                                                        uint32_t scap) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_all[];
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t slot = xcd_slot(blockIdx.x, gridDim.x) * (blockDim.x >> 6) + wave;
    if (blockIdx.x == 0 && threadIdx.x < 3 && b.zero_next) b.zero_next[threadIdx.x] = 0u;      /* (as pya_bin_spectra_kernel) */
    if (slot >= n_ids) return;
    unsigned char *lds_raw = lds_all + (size_t)wave * PYA_BIN_SEL_BYTES(scap);
    const uint32_t psm = psm_ids[slot];
    int status;
    const int R = bin_select<MZ, IT>(b, psm, lds_raw, scap, &status);
    if (R == PYA_BIN_REDO) {
        if (lane_id() == 0) b.redo_ids[atomicAdd(b.redo_count, 1u)] = psm;
        return;
    }
    if (R < 0) bin_store(b, psm, R, status, nullptr, nullptr);
}

/* the spectra the kernels above declined, one per wavefront, a fixed grid striding over the list */
template <typename MZ, typename IT>
__global__ __launch_bounds__(64) void pya_bin_exact_kernel(BatchDev b, uint32_t cap) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_all[];
    const uint32_t n = *b.redo_count;
    for (uint32_t k = blockIdx.x; k < n; k += gridDim.x) {
        const uint32_t psm = b.redo_ids[k];
        const float *r_mz;
        const uint8_t *r_rank;
        int status;
        const int R = bin_core<true, MZ, IT>(b, psm, lds_all, cap, &r_mz, &r_rank, &status);
        bin_store(b, psm, R, status, r_mz, r_rank);
        wave_lds_sync();
    }
}

/* Spectra of more than 8 192 peaks (up to 65 535: 16-bit peak indices): the general body with its arrays in a scratch
 * area of the workspace instead of LDS, one spectrum per wavefront.  Slow (every array access is a trip to memory)
 * and rare; the PSMs behind such spectra are scored by the general kernel, which reads the retained table from the
 * workspace like this kernel leaves it. */
template <typename MZ, typename IT>
__global__ __launch_bounds__(64) void pya_bin_global_kernel(BatchDev b, const uint32_t *ids, uint32_t n_ids, unsigned char *scratch,
                                                            uint64_t stride, uint32_t cap) {
    if (blockIdx.x >= n_ids) return;
    const uint32_t psm = ids[blockIdx.x];
    const float *r_mz;
    const uint8_t *r_rank;
    int status;
    const int R = bin_exact<true, MZ, IT>(b, psm, scratch + (size_t)blockIdx.x * stride, cap, &r_mz, &r_rank, &status);
    bin_store(b, psm, R, status, r_mz, r_rank);
}

/* Shared spectra (pya_plan_create_shared; the hit_depth loop of the reference's __main__.py scores every hit of a scan
 * against the same spectrum): the kernels above then run over spectrum ids and leave ret_n and the binning status per
 * SPECTRUM.  This gives every PSM its spectrum's two words, after the whole binning family (the exact and the global
 * kernel included) and before the first scoring launch, whose prologues read ret_n[psm] and status[psm] without an
 * indirection.  spec_of[psm] == ~0u: set aside by the host pre-pass, no spectrum was binned for it and its status stays. */
__global__ __launch_bounds__(256) void pya_fan_out_kernel(const uint32_t *spec_of, const uint32_t *spec_ret_n, const int32_t *spec_status,
                                                          uint32_t *ret_n, int32_t *status, uint32_t n_psm) {
    const uint32_t psm = blockIdx.x * 256u + threadIdx.x;
    if (psm >= n_psm) return;
    const uint32_t s = spec_of[psm];
    if (s == 0xffffffffu) return;
    ret_n[psm] = spec_ret_n[s];
    status[psm] = spec_status[s];
}

extern "C" int pya_launch_fan_out(const uint32_t *d_spec_of, const uint32_t *d_spec_ret_n, const int32_t *d_spec_status, uint32_t *d_ret_n,
                                  int32_t *d_status, uint32_t n_psm, hipStream_t stream) {
    if (n_psm == 0) return 0;
    hipLaunchKernelGGL(pya_fan_out_kernel, dim3((n_psm + 255u) / 256u), dim3(256), 0, stream, d_spec_of, d_spec_ret_n, d_spec_status,
                       d_ret_n, d_status, n_psm);
    return (int)hipGetLastError();
}

/* The launchers take the element types of b->mz / b->inten (common.h: PYA_SPEC_*) and launch that instantiation; a value
 * that names none is refused -- there is no kernel to fall back to. */
#define PYA_BY_TYPES(types, fn, ...)                                            \
    ((types) == PYA_SPEC_F64_F64   ? fn<double, double>(__VA_ARGS__)            \
     : (types) == PYA_SPEC_F64_F32 ? fn<double, float>(__VA_ARGS__)             \
     : (types) == PYA_SPEC_F32_F32 ? fn<float, float>(__VA_ARGS__)              \
                                   : (int)hipErrorInvalidValue)

extern "C" size_t pya_bin_global_scratch_bytes(uint32_t cap) { return PYA_BIN_WAVE_BYTES(cap); }

template <typename MZ, typename IT>
static int launch_bin_global(const BatchDev *b, const uint32_t *d_ids, uint32_t n_ids, unsigned char *d_scratch, uint64_t stride,
                             uint32_t cap, hipStream_t stream) {
    hipLaunchKernelGGL((pya_bin_global_kernel<MZ, IT>), dim3(n_ids), dim3(64), 0, stream, *b, d_ids, n_ids, d_scratch, stride, cap);
    return (int)hipGetLastError();
}
extern "C" int pya_launch_bin_global(const BatchDev *b, const uint32_t *d_ids, uint32_t n_ids, unsigned char *d_scratch,
                                     uint64_t stride, uint32_t cap, uint32_t types, hipStream_t stream) {
    if (n_ids == 0) return 0;
    return PYA_BY_TYPES(types, launch_bin_global, b, d_ids, n_ids, d_scratch, stride, cap, stream);
}

extern "C" size_t pya_bin_lds_bytes(uint32_t cap) { return PYA_BIN_FAST_BYTES(cap); }

template <typename MZ, typename IT>
static int launch_bin(const BatchDev *b, const uint32_t *d_ids, uint32_t n_ids, uint32_t cap, hipStream_t stream) {
    const size_t per_wave = PYA_BIN_FAST_BYTES(cap);
    const uint32_t nw = per_wave * BIN_WAVES <= 64 * 1024 ? BIN_WAVES : 1;
    size_t lds = nw * per_wave;
    hipError_t e = PYA_ENSURE_MAX_LDS((pya_bin_spectra_kernel<MZ, IT>));
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL((pya_bin_spectra_kernel<MZ, IT>), dim3((n_ids + nw - 1) / nw), dim3(64 * nw), lds, stream, *b, d_ids,
                       n_ids, cap);
    return (int)hipGetLastError();
}
extern "C" int pya_launch_bin(const BatchDev *b, const uint32_t *d_ids, uint32_t n_ids, uint32_t cap, uint32_t types,
                              hipStream_t stream) {
    if (n_ids == 0) return 0;
    return PYA_BY_TYPES(types, launch_bin, b, d_ids, n_ids, cap, stream);
}

extern "C" size_t pya_bin_select_lds_bytes(uint32_t scap) { return PYA_BIN_SEL_BYTES(scap); }

/* scap: survivor slots per spectrum (a multiple of 32) */
template <typename MZ, typename IT>
static int launch_bin_select(const BatchDev *b, const uint32_t *d_ids, uint32_t n_ids, uint32_t scap, hipStream_t stream) {
    const size_t per_wave = PYA_BIN_SEL_BYTES(scap);
    const uint32_t nw = per_wave * BIN_WAVES <= 64 * 1024 ? BIN_WAVES : 1;
    hipError_t e = PYA_ENSURE_MAX_LDS((pya_bin_select_kernel<MZ, IT>));
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL((pya_bin_select_kernel<MZ, IT>), dim3((n_ids + nw - 1) / nw), dim3(64 * nw), nw * per_wave, stream, *b, d_ids, n_ids,
                       scap);
    return (int)hipGetLastError();
}
extern "C" int pya_launch_bin_select(const BatchDev *b, const uint32_t *d_ids, uint32_t n_ids, uint32_t scap, uint32_t types,
                                     hipStream_t stream) {
    if (n_ids == 0) return 0;
    return PYA_BY_TYPES(types, launch_bin_select, b, d_ids, n_ids, scap, stream);
}

template <typename MZ, typename IT>
static int launch_bin_exact(const BatchDev *b, uint32_t n_total, uint32_t cap, hipStream_t stream) {
    const size_t per_wave = PYA_BIN_WAVE_BYTES(cap);
    hipError_t e = PYA_ENSURE_MAX_LDS((pya_bin_exact_kernel<MZ, IT>));
    if (e != hipSuccess) return (int)e;
    const uint32_t grid = n_total < 16384u ? n_total : 16384u;   /* all spectra may need it (count-like intensities) */
    hipLaunchKernelGGL((pya_bin_exact_kernel<MZ, IT>), dim3(grid), dim3(64), per_wave, stream, *b, cap);
    return (int)hipGetLastError();
}
/* after every pya_launch_bin of a batch, with their types: the spectra they declined (b->redo_count must have been
 * zeroed before the first of them) */
extern "C" int pya_launch_bin_exact(const BatchDev *b, uint32_t n_total, uint32_t cap, uint32_t types, hipStream_t stream) {
    if (n_total == 0) return 0;
    return PYA_BY_TYPES(types, launch_bin_exact, b, n_total, cap, stream);
}
