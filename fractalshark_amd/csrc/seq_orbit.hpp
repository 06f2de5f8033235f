// seq_orbit.hpp -- the waypoint cursor: sequential access to a PerturbExtras::SimpleCompression orbit that stays compressed in
// HBM.  Device code shared by the literal LAv2 kernel (kernels_lav2_lit.hip) and the Feature Finder's evaluator (kernels_feature.hip).
//
// The device twin of GPUPerturbSingleResults::SeqWorkspace / GetIterSeq / BinarySearch (Perturb.cuh:160-326) and of the CPU
// RuntimeDecompressor (PerturbationResultsHelpers.h:35-199).  A cursor holds one orbit value; seek() starts from the
// last waypoint at or before the index and iterates z = z^2 + c forward in T arithmetic (c = OrbitXLow / OrbitYLow),
// step() moves one index on: the next waypoint when its index comes up, one iteration otherwise.  Same operations in
// the same order as k_decompress_orbit_* (which expand the same waypoints once per upload), so both modes see the same
// orbit bit for bit; this one trades ~60 vector instructions per step for an orbit that occupies only its waypoints.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/fs_layout.h"
#include "hdr_math.hpp"

namespace fs {

template <class F> struct FsWaypoints;
template <> struct FsWaypoints<float> {
    using Rec = fs_orbit_hdr32_rc;
};
template <> struct FsWaypoints<double> {
    using Rec = fs_orbit_hdr64_rc;
};

// PosT = the reference's IterType for orbit POSITIONS: uint32_t, or uint64_t in the instantiation that counts in 64 bits --
// a compressed orbit can have 2^32 and more uncompressed entries (its waypoints are what is resident), and waypoint
// indices, the cursor, RefIteration and the period are then 64-bit like the reference's (Perturb.cuh:21-23,202-203,247-271).
template <class F, class PosT = uint32_t> struct SeqOrbit {
    const typename FsWaypoints<F>::Rec *__restrict__ wp;
    uint32_t n_wp;
    hreal<F> cx, cy;
    // cursor
    PosT idx;        // orbit index of (zx, zy)
    uint32_t next;   // number of the first waypoint behind the cursor
    PosT next_index; // ... and its orbit index (all ones: none left)
    hreal<F> zx, zy;

    __device__ __forceinline__ PosT index_of(uint32_t k) const
    {
        return (PosT)(wp[k].index_and_rebase & 0x7FFFFFFFFFFFFFFFull);
    }
    __device__ __forceinline__ void load(uint32_t k)
    {
        zx = hreal<F>{wp[k].mx, wp[k].ex};
        zy = hreal<F>{wp[k].my, wp[k].ey};
    }
    __device__ __forceinline__ void step()
    {
        idx++;
        if (idx == next_index) { // GetCompressedComplexSeq, Perturb.cuh:303-326
            load(next);
            next++;
            next_index = next < n_wp ? index_of(next) : ~(PosT)0;
        } else { // runOneIter, PerturbationResultsHelpers.h:51-58
            const hreal<F> zx_old = zx;
            zx = hr_add(hr_sub(hr_mul(zx, zx), hr_mul(zy, zy)), cx);
            hr_reduce(zx);
            zy = hr_add(hr_mul(hr_mul(hreal<F>{F(1), 1}, zx_old), zy), cy);
            hr_reduce(zy);
        }
    }
    __device__ __forceinline__ void seek(PosT i)
    {
        // BinarySearch, Perturb.cuh:241-263: the last waypoint whose index is <= i (waypoint 0 sits at index 0)
        uint32_t lo = 0, hi = n_wp;
        while (hi - lo > 1u) {
            const uint32_t mid = (lo + hi) >> 1;
            if (index_of(mid) <= i)
                lo = mid;
            else
                hi = mid;
        }
        load(lo);
        idx = index_of(lo);
        next = lo + 1u;
        next_index = next < n_wp ? index_of(next) : ~(PosT)0;
        while (idx < i)
            step();
    }
    // seek(0) without the search: waypoint 0 sits at index 0
    __device__ __forceinline__ void rewind()
    {
        load(0u);
        idx = 0;
        next = 1u;
        next_index = next < n_wp ? index_of(next) : ~(PosT)0;
    }
    // PerturbationResults::GetComplex on the cursor's value
    __device__ __forceinline__ hcplx<F> value() const { return hc_from_hr(zx, zy); }
};

} // namespace fs
