// sorter_circuit_common.cuh — the tail kernel the four region-major sorter circuits share (decommit sorter, events / L1 messages
// sorter, log demuxer, storage sorter). A circuit describes itself to it with a traits struct C at the bottom of its kernel header:
//   Job; G, L, MULT_COL, BOUNDARY_ROWS, LOOKUPS_PER_CYCLE; boundary_row(capacity), region_stride(capacity), min_rows(capacity);
//   row0_extra(): the lookup cells outside the cycles' rows that a fill kernel already counted in job.hist;
//   boundary_block(job, capacity, n_rows): the register rows and the closed-form section.
#pragma once
#include "ram_circuit_kernels.cuh"

namespace zkw {

// the boundary rows' cells, zeroed by the boundary block before it fills them (the tail's other blocks zero the rows BELOW them)
template <int COLS, int ROWS>
__device__ __forceinline__ void zero_boundary_rows(u64* trace, size_t n_rows, size_t bnd) {
    for (int k = threadIdx.x; k < COLS * ROWS; k += CF_THREADS) trace[(size_t)(k / ROWS) * n_rows + (bnd + k % ROWS)] = 0;
}

// the boundary rows, the zero padding below them and the multiplicity column
// (k_ram_fill_tail stays apart: it has no boundary block, zeroes only, and is launched only for dirty slots)
template <class C>
static __device__ __forceinline__ void k_sorter_fill_tail(const VB& vb, const typename C::Job* __restrict__ jobs, u32 n_jobs, u32 capacity, size_t n_rows) {
    // 1-D grid: the first n_jobs blocks fill the boundary rows of one trace each (dispatched first and at raised priority: a chain of a dozen
    // dependent permutations that the other blocks' stores hide), then (G + L + 1) * TAIL_CHUNKS blocks per trace
    if (vb.x < n_jobs) {
        __builtin_amdgcn_s_setprio(3);
        C::boundary_block(jobs[vb.x], capacity, n_rows);
        return;
    }
    constexpr u32 PER_JOB = (C::G + C::L + 1) * TAIL_CHUNKS;
    const u32 bid = (vb.x - n_jobs) % PER_JOB;
    const typename C::Job& job = jobs[(vb.x - n_jobs) / PER_JOB];
    u64* trace = job.trace;
    const int col = bid / TAIL_CHUNKS, ch = bid % TAIL_CHUNKS;
    if (col < C::G + C::L) {
        if (job.tail_clean) return;
        const size_t bnd = C::boundary_row(capacity) + C::BOUNDARY_ROWS;  // (BOUNDARY_ROWS is even: 16-byte stores)
        const size_t n_pairs = (n_rows - bnd) / 2;
        const size_t per = (n_pairs + TAIL_CHUNKS - 1) / TAIL_CHUNKS, lo = ch * per, hi = lo + per < n_pairs ? lo + per : n_pairs;
        ulonglong2* c2 = reinterpret_cast<ulonglong2*>(trace + (size_t)col * n_rows + bnd);
        const ulonglong2 z = make_ulonglong2(0, 0);
        for (size_t k = lo + threadIdx.x; k < hi; k += 256) c2[k] = z;
        return;
    }
    u64* mlt = trace + (size_t)C::MULT_COL * n_rows;
    const size_t per = (n_rows + TAIL_CHUNKS - 1) / TAIL_CHUNKS, lo = ch * per, hi = lo + per < n_rows ? lo + per : n_rows;
    for (size_t r = lo + threadIdx.x; r < (job.tail_clean && hi > 256 ? (lo < 256 ? 256 : lo) : hi); r += 256) {  // (a clean slot: rows >= 256 of the column are still zero)
        u64 v = 0;
        if (r < 256) {
            v = job.hist[r];
            if (r == 0) v += (u64)C::L * n_rows - (u64)C::LOOKUPS_PER_CYCLE * capacity - C::row0_extra();
        }
        mlt[r] = v;
    }
}

}  // namespace zkw
