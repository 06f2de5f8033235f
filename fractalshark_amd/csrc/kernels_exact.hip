// kernels_exact.hip -- the exact renderer (fs_render_exact, fs_exact_stable_mask): fixed-point escape counts, one lane per sample,
// no reference orbit and no rounding anywhere (exact_math.hpp holds the arithmetic and the limb bound).
//
// A frame advances in slices of at most `slice` steps per lane.  Between slices the running samples live in device memory as
// (x, y, n, pixel) -- an FsExactList of kernels.h -- limb-major: plane l of a list holds limb l of every slot, so a wave's loads
// and stores are contiguous.  A slice reads list A and writes the samples that are still running to list B: a ballot and a prefix
// count inside the wave, ONE atomic add per wave for the wave's block of slots.  The next slice then runs full waves instead of one
// slow lane per wave.
// A sample that finishes writes its count into the frame at once.  c never changes: the lanes read their column's cx and their
// row's cy (limb-major arrays of the whole axes) at the start of every slice.
//
// Counting: n is the index of the z the lane holds (z_1 = c).  The test comes first: an escape at n leaves n - 1; a z_{N+1} that
// has not escaped leaves N.  That is min(E - 1, N) of every other path.
//
// Sample mode (S = true; fs_exact_audit): the list is n runs of their own instead of a frame's pixels -- run e reads cx[l * n + e]
// and cy[l * n + e] (A.W = A.H = n, the addressing of the wide kernel's W == 0) and leaves its count as uint64 in counts[e]
// (A.iters).  Step loop, slices, compaction and statistics are the frame mode's, which compiles to what it was without the flag.
//
// Cycle check (C = true; fs_set_exact_cycle_check, exact_cycle_math.hpp holds the rule and its proof): a sample whose state repeats
// its checkpoint limb for limb never escapes; it leaves the cap at once and 1 in proved[pixel] (sample mode: proved[e]).  The
// checkpoint is 2L more limb planes per list, the lane's slot of the SOURCE list while the slice runs: written there when it is
// taken, read back only when the two-register fingerprint matches, and copied to the destination slot with the rest of the state by
// a lane that goes on to the next slice.  C = false compiles to what it was without the parameter.
//
// Keeping (K = true; fs_set_exact_keep, frames only): a sample that stops at n == cap + 1 unproved is PARKED (exact_cycle_math.hpp
// says what that state is): it writes the cap into the frame as ever and its state to the park list, at a slot taken the way the
// survivors take theirs -- ballot, prefix count, one atomic add per wave -- from a counter of its own.  Every sample starts at n = 1
// and a slice advances every running lane by the same number of steps, so all running samples hold the same n: they meet the cap in
// one and the same slice, the last one, which has no survivor, and the host hands that slice's unused destination list in as the
// park list (without compaction, a list of its own).  A.resume: the source list holds parked samples, which make their deferred n++
// and cycle check (fsx::cycle_resume) before the step loop.  K = false compiles to what it was without the parameter.
//
// Period planes (P = true; fs_set_exact_periods, frames only, never with K; exact_atom_math.hpp holds the rule): every state that
// passes the escape test with n <= cap hands its norm x^2 + y^2 -- the sum the escape test was made on -- to the rule, which keeps the
// smallest per PIXEL: 2L limb planes of W * H, a key plane and the plane of the index it was taken at, A.atom.  State per pixel, not
// per slot: the lists carry nothing new and compaction copies nothing new.  The lane holds the minimum's 64-bit key in two registers
// (reloaded from the key plane at the start of a slice) and touches memory only when it takes a new minimum or the keys are equal.
// With C, a proved sample also leaves n - t in A.cyclen.  P = false compiles to what it was without the parameter.
//
// Point runs (S = true and P = true, never with C or K; fs_exact_eval_points): a list of runs, the period state per RUN (sample
// mode's addressing, W = H = n runs), and two things more.  Run e stops at A.lengths[e] where a frame stops at A.cap: cap + 1, which
// the P kernels hold in a vector register, is lengths[e] + 1.  And the state that passes the escape test with n == lengths[e] goes to
// the end planes (fsx::point_end): plain vector stores, once per run, before the step advances the state.  Runs of different lengths
// leave the list at different slices; the compaction closes the gaps as it does behind escapes.
#include <hip/hip_runtime.h>

#include "exact_atom_math.hpp"
#include "kernels.h"

namespace {

// a finished sample's count goes to the frame (sample mode: to counts[e])
template <bool S> __device__ __forceinline__ void write_count(const FsExactArgs &A, size_t out_idx, uint64_t v)
{
    if (S || A.iter_u64)
        ((uint64_t *)A.iters)[out_idx] = v;
    else
        ((uint32_t *)A.iters)[out_idx] = (uint32_t)v;
}

template <int L, bool S, bool C, bool K, bool P> __global__ void __launch_bounds__(64) k_exact_slice(const FsExactArgs A)
{
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    bool alive = i < A.n_src;
    const uint32_t slot = alive ? i : 0u; // (a lane beyond the list reads slot 0 and writes nothing)
    uint64_t n = 1;
    uint32_t pix = slot;
    if (!A.first) {
        n = A.src.n[slot];
        pix = A.src.id[slot];
        alive = alive && n != 0; // (without compaction a finished sample keeps its slot, marked n = 0)
    }
    if (__ballot(alive) == 0)
        return;
    const uint32_t col = S ? pix : pix % A.W, row = S ? pix : pix / A.W;
    uint32_t x[L], y[L], cx[L], cy[L];
#pragma unroll
    for (int l = 0; l < L; l++) {
        cx[l] = A.cx[(size_t)l * A.W + col];
        cy[l] = A.cy[(size_t)l * A.H + row];
    }
    if (A.first) {
#pragma unroll
        for (int l = 0; l < L; l++)
            x[l] = cx[l], y[l] = cy[l];
    } else {
#pragma unroll
        for (int l = 0; l < L; l++) {
            x[l] = A.src.xy[(size_t)l * A.stride + slot];
            y[l] = A.src.xy[(size_t)(L + l) * A.stride + slot];
        }
    }

    // the checkpoint: this lane's slot of the source list's planes (a running lane's slot is i); its low limbs stay in registers
    uint32_t fx = 0, fy = 0, my_compares = 0, my_proved = 0;
    if constexpr (C) {
        if (A.first) {
            if (alive)
                fsx::cycle_take<L>(x, y, A.src.ck, A.stride, i, fx, fy);
        } else {
            fx = A.src.ck[slot], fy = A.src.ck[(size_t)L * A.stride + slot];
        }
    }

    // the key of the pixel's smallest norm so far (first slice: none yet, and the take at n = 1 asks for none)
    uint64_t kmin = 0, cap1 = 0;
    uint32_t atom_compares = 0, key_shift = 0; // (the read-backs are not reported)
    if constexpr (P) {
        if (!A.first)
            kmin = A.periods->keys[pix];
        key_shift = A.atom_key_shift, cap1 = (S ? A.lengths[pix] : A.cap) + 1;
        FSX_PIN(key_shift); // (vector registers: the scalar ones are what the largest instantiations run out of)
        FSX_PIN(cap1);
    }

    const size_t out_idx = S ? (size_t)pix : (size_t)row * A.rounded_width + col;
    uint32_t my_steps = 0, wave_steps = 0;
    bool parked = false;
    if constexpr (K) {
        if (A.resume && alive) {
            if (fsx::cycle_resume<L, C>(x, y, n, A.src.ck, A.stride, i, fx, fy, A.fp_mx, A.fp_my, my_compares)) {
                write_count<S>(A, out_idx, A.cap);
                A.proved[pix] = 1;
                my_proved = 1;
                alive = false;
            }
        }
    }
    for (uint32_t k = 0; k < A.slice; k++) {
        if (__ballot(alive) == 0)
            break;
        wave_steps++;
        if (alive) {
            my_steps++;
            bool escaped;
            if constexpr (P) {
                // The limb offset of the floor shift in a vector register, made anew every step: as a loop invariant its L
                // comparisons are L scalar register pairs held across the whole loop, and with this rule's own conditions the
                // instantiations from L = 18 then spill scalar registers.  From there on the limb position of the bailout goes the
                // same way (2L more invariants, the limbs the norm is compared with).
                fsx::Params Pq = A.P;
                FSX_PIN(Pq.q);
                if constexpr (L >= 18) {
                    FSX_PIN(Pq.bail_q);
                    FSX_PIN(Pq.bail_lo);
                    FSX_PIN(Pq.bail_hi);
                    FSX_PIN(Pq.r);
                }
                escaped = fsx::step_with<L>(
                    x, y, cx, cy, Pq, [&](const uint32_t(&xx)[2 * L], const uint32_t(&yy)[2 * L], const uint32_t(&w)[2 * L]) {
                        if constexpr (S) {
                            if (n + 1 == cap1)
                                fsx::point_end<L>(x, y, A.periods, pix);
                        }
                        // (z_{cap+1} is tested, not tracked)
                        fsx::atom_track<L>(xx, yy, w, n, n != cap1, A.periods, pix, kmin, key_shift, atom_compares);
                    });
            } else {
                escaped = fsx::step<L>(x, y, cx, cy, A.P);
            }
            if (escaped || n == (P ? cap1 : A.cap + 1)) {
                write_count<S>(A, out_idx, escaped ? n - 1 : (S && P ? cap1 - 1 : A.cap));
                alive = false;
                if constexpr (K)
                    parked = !escaped;
            } else {
                n++;
                if constexpr (C) {
                    if (fsx::cycle_check<L>(x, y, n, A.src.ck, A.stride, i, fx, fy, A.fp_mx, A.fp_my, my_compares)) {
                        write_count<S>(A, out_idx, A.cap);
                        uint32_t p = pix;
                        FSX_PIN(p); // (the address is made here, not kept across the loop)
                        A.proved[p] = 1;
                        if constexpr (P) {
                            const fsx::AtomPlanes *planes = A.periods;
                            FSX_PIN(planes);
                            planes->cyclen[p] = fsx::cycle_length(n);
                        }
                        my_proved = 1;
                        alive = false;
                    }
                }
            }
        }
    }

    // the samples still running go to the next slice's list
    const uint64_t live = __ballot(alive);
    const uint32_t n_live = (uint32_t)__popcll(live);
    uint32_t dst = i;
    if (A.compact) {
        uint32_t base = 0;
        if (threadIdx.x == 0 && n_live != 0)
            base = atomicAdd(A.dst_count, n_live);
        base = __shfl(base, 0);
        dst = base + (uint32_t)__popcll(live & ((1ull << threadIdx.x) - 1ull));
    } else if (threadIdx.x == 0 && n_live != 0) {
        atomicAdd(A.dst_count, n_live);
    }
    if (alive) {
#pragma unroll
        for (int l = 0; l < L; l++) {
            A.dst.xy[(size_t)l * A.stride + dst] = x[l];
            A.dst.xy[(size_t)(L + l) * A.stride + dst] = y[l];
        }
        A.dst.n[dst] = n;
        A.dst.id[dst] = pix;
        if constexpr (C) {
            if (A.compact) { // (without compaction source and destination are one list and dst == slot)
#pragma unroll
                for (int l = 0; l < 2 * L; l++)
                    A.dst.ck[(size_t)l * A.stride + dst] = A.src.ck[(size_t)l * A.stride + i];
            }
        }
    } else if (!A.compact && i < A.n_src) {
        A.dst.n[dst] = 0;
        A.dst.id[dst] = 0;
    }

    // the samples that met the cap go to the park list
    if constexpr (K) {
        const uint64_t pk = __ballot(parked);
        if (pk != 0) {
            uint32_t base = 0;
            if (threadIdx.x == 0)
                base = atomicAdd(A.park_count, (uint32_t)__popcll(pk));
            base = __shfl(base, 0);
            const uint32_t ps = base + (uint32_t)__popcll(pk & ((1ull << threadIdx.x) - 1ull));
            if (parked) {
#pragma unroll
                for (int l = 0; l < L; l++) {
                    A.park.xy[(size_t)l * A.stride + ps] = x[l];
                    A.park.xy[(size_t)(L + l) * A.stride + ps] = y[l];
                }
                A.park.n[ps] = n;
                A.park.id[ps] = pix;
                if constexpr (C) {
#pragma unroll
                    for (int l = 0; l < 2 * L; l++)
                        A.park.ck[(size_t)l * A.stride + ps] = A.src.ck[(size_t)l * A.stride + i];
                }
            }
        }
    }

    // lane slots the wave occupied in its step loop, and the steps its lanes really took
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        my_steps += __shfl_xor(my_steps, off);
    if (threadIdx.x == 0) {
        atomicAdd(&A.stats[0], 64ull * wave_steps);
        atomicAdd(&A.stats[1], (unsigned long long)my_steps);
    }
    if constexpr (C) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            my_proved += __shfl_xor(my_proved, off);
            my_compares += __shfl_xor(my_compares, off);
        }
        if (threadIdx.x == 0) {
            if (my_proved)
                atomicAdd(&A.stats[2], (unsigned long long)my_proved);
            if (my_compares)
                atomicAdd(&A.stats[3], (unsigned long long)my_compares);
        }
    }
}

// a continuation's proved pixels take the new cap
template <class T>
__global__ void __launch_bounds__(256) k_exact_set_proved(T *__restrict__ iters, const uint8_t *__restrict__ proved, uint32_t W, uint32_t H,
                                                           uint32_t pitch, T value)
{
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p < W * H && proved[p])
        iters[(size_t)(p / W) * pitch + p % W] = value;
}

template <class T>
__global__ void __launch_bounds__(256) k_exact_mask(const T *__restrict__ centre, const T *__restrict__ shifted, uint8_t *__restrict__ mask,
                                                     uint32_t W, uint32_t H, uint32_t pitch, int first)
{
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= W * H)
        return;
    const size_t idx = (size_t)(p / W) * pitch + p % W;
    const uint8_t same = centre[idx] == shifted[idx] ? 1 : 0;
    mask[p] = first ? same : (uint8_t)(mask[p] & same);
}

} // namespace

bool fsk_exact_slice(const FsExactArgs &A, uint32_t limbs, bool samples, bool cycle, bool keep, bool periods, hipStream_t s)
{
    if ((keep && samples) || (periods && keep) || (periods && samples && cycle))
        return false;
    const dim3 grid((A.n_src + 63u) / 64u), block(64);
    switch (limbs) {
#define FS_EXACT_CASE(L)                                                                                                \
    case L:                                                                                                             \
        if (periods && samples)                                                                                         \
            hipLaunchKernelGGL((k_exact_slice<L, true, false, false, true>), grid, block, 0, s, A);                     \
        else if (periods && cycle)                                                                                      \
            hipLaunchKernelGGL((k_exact_slice<L, false, true, false, true>), grid, block, 0, s, A);                     \
        else if (periods)                                                                                               \
            hipLaunchKernelGGL((k_exact_slice<L, false, false, false, true>), grid, block, 0, s, A);                    \
        else if (keep && cycle)                                                                                         \
            hipLaunchKernelGGL((k_exact_slice<L, false, true, true, false>), grid, block, 0, s, A);                     \
        else if (keep)                                                                                                  \
            hipLaunchKernelGGL((k_exact_slice<L, false, false, true, false>), grid, block, 0, s, A);                    \
        else if (cycle && samples)                                                                                      \
            hipLaunchKernelGGL((k_exact_slice<L, true, true, false, false>), grid, block, 0, s, A);                     \
        else if (cycle)                                                                                                 \
            hipLaunchKernelGGL((k_exact_slice<L, false, true, false, false>), grid, block, 0, s, A);                    \
        else if (samples)                                                                                               \
            hipLaunchKernelGGL((k_exact_slice<L, true, false, false, false>), grid, block, 0, s, A);                    \
        else                                                                                                            \
            hipLaunchKernelGGL((k_exact_slice<L, false, false, false, false>), grid, block, 0, s, A);                   \
        return true;
        FS_EXACT_FOR_EACH_L(FS_EXACT_CASE)
#undef FS_EXACT_CASE
    default:
        return false;
    }
}

void fsk_exact_set_proved(void *iters, int iter_u64, const uint8_t *proved, uint32_t W, uint32_t H, uint32_t pitch, uint64_t value,
                          hipStream_t s)
{
    const dim3 grid((W * H + 255u) / 256u), block(256);
    if (iter_u64)
        hipLaunchKernelGGL(k_exact_set_proved<uint64_t>, grid, block, 0, s, (uint64_t *)iters, proved, W, H, pitch, value);
    else
        hipLaunchKernelGGL(k_exact_set_proved<uint32_t>, grid, block, 0, s, (uint32_t *)iters, proved, W, H, pitch, (uint32_t)value);
}

void fsk_exact_mask(const void *centre, const void *shifted, int iter_u64, uint8_t *mask, uint32_t W, uint32_t H, uint32_t pitch,
                    int first, hipStream_t s)
{
    const dim3 grid((W * H + 255u) / 256u), block(256);
    if (iter_u64)
        hipLaunchKernelGGL(k_exact_mask<uint64_t>, grid, block, 0, s, (const uint64_t *)centre, (const uint64_t *)shifted, mask, W, H,
                           pitch, first);
    else
        hipLaunchKernelGGL(k_exact_mask<uint32_t>, grid, block, 0, s, (const uint32_t *)centre, (const uint32_t *)shifted, mask, W, H,
                           pitch, first);
}
