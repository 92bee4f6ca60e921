// gs_filter.hip -- the Bloom filter of the filter goal on the device.
//
// filter: one wave per read, lanes = k-mer positions, the reference's exact Bloom hashes; accept is the
// closed form  #(member k-mers) >= max(posThreshold, 1)  of FastqBloomFilter.isAcceptRead (:120-161).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gs_absmod.h"  // gs_absmod: the filter's bit index; gs_murmur64
#include "gs_launch.h"
#include "gs_layout.h"
#include "gs_params.h"
#include "gs_wave.h"

// ---------------------------------------------------------------------------------------------------
// filter
// ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ u64 gs_spread32(uint32_t v) {  // bit i -> bit 2i
    u64 x = v;
    x = (x | (x << 16)) & 0x0000FFFF0000FFFFULL;
    x = (x | (x << 8)) & 0x00FF00FF00FF00FFULL;
    x = (x | (x << 4)) & 0x0F0F0F0F0F0F0F0FULL;
    x = (x | (x << 2)) & 0x3333333333333333ULL;
    x = (x | (x << 1)) & 0x5555555555555555ULL;
    return x;
}

// canonical k-mer in the REFERENCE's interleaved encoding (the value the Bloom hashes see)
__device__ __forceinline__ int64_t gs_canonical_java(uint32_t fhi, uint32_t flo, int k, uint32_t kmask) {
    const uint32_t rhi = __brev(fhi) >> (32 - k);
    const uint32_t rlo = __brev(flo) >> (32 - k);
    const u64 fwd = (gs_spread32(rhi) << 1) | gs_spread32(rlo);                     // first base in the top bits
    const u64 rev = (gs_spread32(fhi) << 1) | gs_spread32((flo ^ kmask) & kmask);   // complement, reversed
    return (int64_t)(fwd > rev ? fwd : rev);
}

// bit `i`-th hash of `key` in the filter (XOR or Murmur kind); factors come from the block's LDS copy
__device__ __forceinline__ bool gs_filter_bit(const GsFilterParams &P, const uint32_t *words32, const int64_t *factors,
                                              int64_t key, int i) {
    const int64_t f = factors[i];
    const int64_t h = P.kind == GS_BLOOM_XOR ? (f ^ key) : gs_murmur64(key, f);
    const u64 idx = gs_absmod(h, P.bits, P.magic, P.magic_shift);
    return ((words32[(uint32_t)(idx >> 5)] >> (idx & 31)) & 1u) != 0;
}

#define GS_FILTER_MAX_HASHES 128

__global__ __launch_bounds__(GS_BLOCK) __attribute__((amdgpu_waves_per_eu(GS_WAVES, GS_WAVES))) void gs_filter_kernel(GsFilterParams P) {
    __shared__ u64 s_fkey[GS_BLOCK / 64][16];
    __shared__ u64 s_fcand[GS_BLOCK / 64][64];
    __shared__ int64_t s_factors[GS_FILTER_MAX_HASHES];
    for (int i = threadIdx.x; i < P.n_hashes && i < GS_FILTER_MAX_HASHES; i += blockDim.x) s_factors[i] = P.factors[i];
    __syncthreads();
    const int lane = gs_lane();
    const int wave_in_block = threadIdx.x >> 6;
    const int64_t wave_id = (int64_t)blockIdx.x * (GS_BLOCK / 64) + (threadIdx.x >> 6);
    const int64_t n_waves = (int64_t)gridDim.x * (GS_BLOCK / 64);
    const int k = P.k;
    const uint32_t kmask = (1u << k) - 1u;
    // bit i of the filter = bit (i & 31) of 32-bit word i >> 5 (little endian): a dword load with a scalar base and a
    // 32-bit lane offset is the cheapest scattered load there is (XOR / Murmur filters are limited to 2^37 bits)
    const uint32_t *words32 = reinterpret_cast<const uint32_t *>(P.words);
    const int64_t n_reads = (P.skip != nullptr && *P.skip != 0) ? 0 : P.n_reads;
    for (int64_t r = wave_id; r < n_reads; r += n_waves) {
        const uint64_t *po = P.off + r * P.off_stride;
        const u64 off = po[0];
        const int L = (int)(po[1] - off);
        const int max = L - k + 1;
        const uint8_t *rd = P.seq + off;
        int accept = 0;
        if (max > 0) {
            const int pos_thr = P.min_pos_count > 0 ? P.min_pos_count : (int)((double)max * P.positive_ratio);
            const int need = pos_thr > 1 ? pos_thr : 1;
            int members = 0;
            u64 hi0, lo0, bad0;
            gs_load_word(rd, L, 0, lane, hi0, lo0, bad0);
            for (int round = 0; round * 64 < max && members < need; round++) {
                u64 hi1, lo1, bad1;
                gs_load_word(rd, L, round + 1, lane, hi1, lo1, bad1);
                const int p = 64 * round + lane;
                const uint32_t fhi = (uint32_t)gs_funnel(hi0, hi1, lane) & kmask;
                const uint32_t flo = (uint32_t)gs_funnel(lo0, lo1, lane) & kmask;
                const uint32_t wbad = (uint32_t)gs_funnel(bad0, bad1, lane) & kmask;
                const bool valid_lane = p < max && wbad == 0;
                const int64_t key = gs_canonical_java(fhi, flo, k, kmask);
                // A read that comes from the indexed genomes is accepted by its first few k-mers, so the first round
                // looks at every 8th position before it pays for all of them: an accepted read then costs ~60 filter
                // lines instead of ~250, a rejected one pays one extra round trip.  Every position is still examined
                // at most once and accept <=> #members >= need is unchanged.
                for (int pass = round == 0 ? 0 : 1; pass < 2 && members < need; pass++) {
                    bool alive = valid_lane && (round != 0 || (((lane & 7) == 0) == (pass == 0)));
                    if (P.kind == GS_BLOOM_BLOCKED) {
                        if (alive) {  // BlockedKMerBloomFilter.containsLong :181-199
                            const int64_t h0 = P.factors[0] ^ key;
                            const u64 start = gs_absmod(h0, P.bits, P.magic, P.magic_shift);
                            u64 uh = (u64)h0;
                            uh ^= (uh << 32) | (uh >> 32);
                            const int64_t sh = (int64_t)uh;
                            const u64 m1 = (1ULL << (sh & 63)) | (1ULL << ((sh >> 6) & 63));
                            const u64 m2 = (1ULL << ((sh >> 12) & 63)) | (1ULL << ((sh >> 18) & 63));
                            const u64 a = P.words[start];
                            const u64 b = P.words[start + 1 + (uh >> 60)];
                            alive = ((m1 & a) == m1) && ((m2 & b) == m2);
                        }
                    } else {
                        // AbstractKMerBloomFilter.containsLong :209-216.  accept <=> #members >= need, and a member is a
                        // k-mer whose n_hashes bits are all set; in which order the bits are looked at is free.  A
                        // scattered load costs the CU about the same whether 1 or 64 lanes take part, so the work is
                        // arranged to keep the lanes of every load busy:
                        //   1. hashes 0..2 per lane (drops ~88 % of the non-members of a half-full filter),
                        //   2. the survivors, 16 at a time, are spread over the wave: 4 lanes per survivor look at
                        //      hashes 3..6 in ONE load (keys travel through LDS),
                        //   3. what is still alive is a candidate: the lanes look at the next 8 hashes of one
                        //      candidate in one load (a false candidate rarely gets further), then at all the rest,
                        //      candidate after candidate until `need` members are confirmed.
                        // Measured on the 47 M-key index filter: 58 -> 12 load instructions and 153 -> ~180 filter
                        // lines per read, 59.8 -> 38.3 ms per 10 M reads; the kernel now runs at the fabric's
                        // random-line rate instead of at the CU's rate of (mostly empty) load instructions.
                        const int nh = P.n_hashes;
                        const int S = 3;  // per-lane steps
                        for (int i = 0; i < S && i < nh && __ballot(alive) != 0; i++) {
                            if (alive) alive = gs_filter_bit(P, words32, s_factors, key, i);
                        }
                        u64 rem = __ballot(alive);
                        int confirmed = 0;
                        if (nh <= S) {
                            confirmed = __popcll(rem);
                            rem = 0;
                        }
                        const int T = nh - S < 4 ? nh - S : 4;
                        int nc = 0, cdone = 0;
                        u64 *fkey = s_fkey[wave_in_block], *fcand = s_fcand[wave_in_block];
                        while (rem != 0 && members + confirmed < need) {
                            const int rank = __popcll(rem & ((1ULL << lane) - 1));
                            const bool in_batch = ((rem >> lane) & 1ULL) && rank < 16;
                            const u64 batch = __ballot(in_batch);
                            const int nb = __popcll(batch);
                            if (in_batch) fkey[rank] = (u64)key;
                            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                            __builtin_amdgcn_wave_barrier();
                            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                            const int j = lane >> 2, t = lane & 3;
                            const bool active = j < nb && t < T;
                            bool bit = true;
                            u64 jkey = 0;
                            if (j < nb) jkey = fkey[j];
                            if (active) bit = gs_filter_bit(P, words32, s_factors, (int64_t)jkey, S + t);
                            const u64 okm = __ballot(bit);
                            u64 pass4 = okm & (okm >> 1) & (okm >> 2) & (okm >> 3) & 0x1111111111111111ULL;
                            pass4 &= nb >= 16 ? ~0ULL : ((1ULL << (4 * nb)) - 1);  // groups beyond the batch are idle
                            if (((pass4 >> lane) & 1ULL) != 0) fcand[nc + __popcll(pass4 & ((1ULL << lane) - 1))] = jkey;
                            nc += __popcll(pass4);
                            rem &= ~batch;
                            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                            __builtin_amdgcn_wave_barrier();
                            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                            while (cdone < nc && members + confirmed < need) {
                                const int64_t ckey = (int64_t)fcand[cdone++];
                                bool all = true;
                                {
                                    const int i = S + T + lane;  // a first slice of 8 hashes
                                    const bool b = (lane < 8 && i < nh) ? gs_filter_bit(P, words32, s_factors, ckey, i) : true;
                                    all = __ballot(b) == ~0ULL;
                                }
                                for (int base = S + T + 8; base < nh && all; base += 64) {
                                    const int i = base + lane;
                                    const bool b = i < nh ? gs_filter_bit(P, words32, s_factors, ckey, i) : true;
                                    all = __ballot(b) == ~0ULL;
                                }
                                confirmed += all ? 1 : 0;
                            }
                            __builtin_amdgcn_wave_barrier();  // fkey / fcand are rewritten by the next batch
                        }
                        members += confirmed;
                        alive = false;  // already counted
                    }
                    members += __popcll(__ballot(alive));
                }
                hi0 = hi1;
                lo0 = lo1;
                bad0 = bad1;
            }
            accept = members >= need;
        }
        if (lane == 0) P.accept[r] = (uint8_t)accept;
    }
}

extern "C" int gs_filter_occupancy() {
    int n = 0;
    hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, gs_filter_kernel, GS_BLOCK, 0);
    return e == hipSuccess ? n : 0;
}

extern "C" hipError_t gs_launch_filter(const GsFilterParams *P, int grid, hipStream_t stream) {
    hipLaunchKernelGGL(gs_filter_kernel, dim3(grid), dim3(GS_BLOCK), 0, stream, *P);
    return hipGetLastError();
}
