// gs_route.hip -- the kernels of the DB-partitioned mode around the two exchanges: reads -> keys (gs_encode_kernel), keys -> owner
// regions (route / unroute), keys -> nodes on the owner (gs_probe_keys_kernel).  The per-read reduce over the routed-back nodes is
// gs_match_kernel<.., FROM_NODES = true> (gs_kernels.hip).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "gs_launch.h"
#include "gs_layout.h"
#include "gs_params.h"
#include "gs_wave.h"

// ---------------------------------------------------------------------------------------------------
// DB-partitioned mode: the fused kernel is split into
//   gs_encode_kernel      reads -> mixed key h of every k-mer position (GS_KEY_INVALID for windows with a bad base,
//                         GS_KEY_MISS for k-mers the store-wide minimizer gate rules out)
//   gs_probe_keys_kernel  keys -> node (value index / miss), run by the rank that OWNS the key's table partition
//   gs_match_kernel<.., FROM_NODES = true>   per-read reduce over the routed-back node stream
// with two all-to-all exchanges in between (genestrip_amd/distributed.py).
// ---------------------------------------------------------------------------------------------------
#define GS_KEY_INVALID (~0ULL)
#define GS_KEY_MISS (~0ULL - 1)  // the minimizer gate already says "not stored": never routed, node = MISS
#define GS_KEY_ROUTED(h) ((h) < GS_KEY_MISS)

template <int KC>
__global__ __launch_bounds__(GS_BLOCK) void gs_encode_kernel(GsEncodeParams P) {
    __shared__ uint32_t s_g[GS_BLOCK / 64][2 * GS_ROW];  // 15-mer order hashes of the wave's current 128 + 16 positions
    const int lane = gs_lane();
    uint32_t *wave_g = s_g[threadIdx.x >> 6];
    const int64_t wave_id = (int64_t)blockIdx.x * (GS_BLOCK / 64) + (threadIdx.x >> 6);
    const int64_t n_waves = (int64_t)gridDim.x * (GS_BLOCK / 64);
    const int k = KC ? KC : P.k;  // KC = compile-time k (0: any k)
    const uint32_t kmask = (1u << k) - 1u;
    // software pipeline over the wave's reads: the first 192 bases of the next read are loaded while the current
    // one is hashed (a read is a chain of dependent loads: offsets -> bases -> gate word)
    u64 off = 0, pb = 0;
    int L = 0;
    uint32_t c[3] = {0, 0, 0};
    if (wave_id < P.n_reads) {
        off = P.off[wave_id];
        L = (int)(P.off[wave_id + 1] - off);
        pb = P.pos_off[wave_id];
#pragma unroll
        for (int i = 0; i < 3; i++) c[i] = 64 * i + lane < L ? P.seq[off + 64 * i + lane] : GS_FILL;
    }
    for (int64_t r = wave_id; r < P.n_reads; r += n_waves) {
        const int max = L - k + 1;
        const uint8_t *rd = P.seq + off;
        const int64_t rn = r + n_waves;
        u64 offN = 0, pbN = 0;
        int LN = 0;
        if (rn < P.n_reads) {
            offN = P.off[rn];
            LN = (int)(P.off[rn + 1] - offN);
            pbN = P.pos_off[rn];
        }
        uint32_t cN[3] = {0, 0, 0};
        for (int base = 0; base < max || base == 0; base += 128) {
            u64 Bhi[3], Blo[3], Bbad[3];
#pragma unroll
            for (int i = 0; i < 3; i++) {
                if (base == 0)
                    gs_word_from_byte(c[i], Bhi[i], Blo[i], Bbad[i]);
                else
                    gs_load_word(rd, L, (base >> 6) + i, lane, Bhi[i], Blo[i], Bbad[i]);
            }
            if (base == 0 && rn < P.n_reads) {
#pragma unroll
                for (int i = 0; i < 3; i++) cN[i] = 64 * i + lane < LN ? P.seq[offN + 64 * i + lane] : GS_FILL;
            }
            if (max <= 0) break;
            u64 key[2];
            uint32_t fhi[2], flo[2];
#pragma unroll
            for (int s = 0; s < 2; s++) {
                fhi[s] = (uint32_t)gs_funnel(Bhi[s], Bhi[s + 1], lane) & kmask;
                flo[s] = (uint32_t)gs_funnel(Blo[s], Blo[s + 1], lane) & kmask;
                const uint32_t wbad = (uint32_t)gs_funnel(Bbad[s], Bbad[s + 1], lane) & kmask;
                key[s] = wbad ? GS_KEY_INVALID : gs_kmer_hash(fhi[s], flo[s], k, kmask);
            }
            if (P.mgate != nullptr) {
                // the store's minimizer gate (which covers the keys of every partition) as in gs_probe_planes: k-mers
                // it rules out are not routed at all
                int mp[2];
                uint32_t cf[2];
                uint32_t rhi[2], rlo[2];
#pragma unroll
                for (int s = 0; s < 2; s++) {
                    rhi[s] = __brev(fhi[s]) >> (32 - k);
                    rlo[s] = (__brev(flo[s]) >> (32 - k)) ^ kmask;
                }
                gs_wave_minimizers<KC>(Bhi, Blo, fhi, flo, rhi, rlo, k, lane, wave_g, mp, cf);
#pragma unroll
                for (int s = 0; s < 2; s++) {
                    if (base + 64 * s + lane < max && key[s] != GS_KEY_INVALID) {
                        const uint32_t gh = gs_canon_hash(cf[s] >> 1);  // only the minimizer's hash is needed
                        const uint32_t bits = gs_mgate_bits(gh);
                        if ((P.mgate[gs_mgate_word(gh, P.mgate_bits)] & bits) != bits) key[s] = GS_KEY_MISS;
                    }
                }
            }
#pragma unroll
            for (int s = 0; s < 2; s++) {
                const int p = base + 64 * s + lane;
                if (p < max) P.keys[pb + (u64)p] = key[s];
            }
        }
        off = offN;
        L = LN;
        pb = pbN;
#pragma unroll
        for (int i = 0; i < 3; i++) c[i] = cN[i];
    }
}

// ---- encode and routing in one pass: what gs_encode_kernel + gs_route_count_kernel + gs_route_scatter_kernel do through
// an 8-byte key per k-mer POSITION that is written once and read twice.  Here a wave appends the keys of its reads
// straight to the owners' send regions: it holds one chunk of GS_ROUTE_CHUNK slots per owner (cursor in LDS), takes a
// new one with a single global atomic when the chunk cannot take a sub-round's keys (the rest of the old chunk becomes
// sentinels), and pads its open chunks at the end.  Keys leave in no particular order inside an owner's region.
template <int KC>
__global__ __launch_bounds__(GS_BLOCK) void gs_encode_route_kernel(GsEncodeParams P, GsRouteParams R) {
    __shared__ uint32_t s_g[GS_BLOCK / 64][2 * GS_ROW];
    __shared__ unsigned long long s_base[GS_BLOCK / 64][64];  // per wave and owner: base of the chunk in hand
    __shared__ uint32_t s_used[GS_BLOCK / 64][64];            // slots used in it (GS_ROUTE_CHUNK: none in hand)
    const int lane = gs_lane();
    const int wv = threadIdx.x >> 6;
    uint32_t *wave_g = s_g[wv];
    const int64_t wave_id = (int64_t)blockIdx.x * (GS_BLOCK / 64) + wv;
    const int64_t n_waves = (int64_t)gridDim.x * (GS_BLOCK / 64);
    const int k = KC ? KC : P.k;
    const uint32_t kmask = (1u << k) - 1u;
    const int n_parts = R.n_parts;
    if (lane < n_parts) {
        s_base[wv][lane] = 0;
        s_used[wv][lane] = GS_ROUTE_CHUNK;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    for (int64_t r = wave_id; r < P.n_reads; r += n_waves) {
        const u64 off = P.off[r];
        const int L = (int)(P.off[r + 1] - off);
        const u64 pb = P.pos_off[r];
        const int max = L - k + 1;
        const uint8_t *rd = P.seq + off;
        for (int base = 0; base < max; base += 128) {
            u64 Bhi[3], Blo[3], Bbad[3];
#pragma unroll
            for (int i = 0; i < 3; i++) gs_load_word(rd, L, (base >> 6) + i, lane, Bhi[i], Blo[i], Bbad[i]);
            u64 key[2];
            uint32_t fhi[2], flo[2];
#pragma unroll
            for (int s = 0; s < 2; s++) {
                fhi[s] = (uint32_t)gs_funnel(Bhi[s], Bhi[s + 1], lane) & kmask;
                flo[s] = (uint32_t)gs_funnel(Blo[s], Blo[s + 1], lane) & kmask;
                const uint32_t wbad = (uint32_t)gs_funnel(Bbad[s], Bbad[s + 1], lane) & kmask;
                key[s] = wbad ? GS_KEY_INVALID : gs_kmer_hash(fhi[s], flo[s], k, kmask);
            }
            if (P.mgate != nullptr) {
                int mp[2];
                uint32_t cf[2];
                uint32_t rhi[2], rlo[2];
#pragma unroll
                for (int s = 0; s < 2; s++) {
                    rhi[s] = __brev(fhi[s]) >> (32 - k);
                    rlo[s] = (__brev(flo[s]) >> (32 - k)) ^ kmask;
                }
                gs_wave_minimizers<KC>(Bhi, Blo, fhi, flo, rhi, rlo, k, lane, wave_g, mp, cf);
#pragma unroll
                for (int s = 0; s < 2; s++) {
                    if (base + 64 * s + lane < max && key[s] != GS_KEY_INVALID) {
                        const uint32_t gh = gs_canon_hash(cf[s] >> 1);
                        const uint32_t bits = gs_mgate_bits(gh);
                        if ((P.mgate[gs_mgate_word(gh, P.mgate_bits)] & bits) != bits) key[s] = GS_KEY_MISS;
                    }
                }
            }
#pragma unroll
            for (int s = 0; s < 2; s++) {
                const int p = base + 64 * s + lane;
                const bool in = p < max;
                const bool routed = in && GS_KEY_ROUTED(key[s]);
                if (in) R.nodes[pb + (u64)p] = key[s] == GS_KEY_INVALID ? GS_NODE_INVALID : GS_NODE_MISS;  // (routed: overwritten later)
                const int owner = routed ? (int)((key[s] >> GS_OWNER_SHIFT) % (u64)n_parts) : -1;
                u64 todo = __ballot(routed);
                while (todo) {  // one owner after the other
                    const int o = gs_readlane(owner, __builtin_ctzll(todo));
                    const u64 mine = __ballot(owner == o);
                    const uint32_t cnt = (uint32_t)__popcll(mine);
                    uint32_t used = s_used[wv][o];
                    u64 cbase = s_base[wv][o];
                    if (used + cnt > GS_ROUTE_CHUNK) {
                        // the rest of the chunk in hand becomes sentinels; a new chunk
                        if (used < GS_ROUTE_CHUNK && cbase + GS_ROUTE_CHUNK <= R.cap)
                            for (uint32_t j = used + (uint32_t)lane; j < GS_ROUTE_CHUNK; j += 64) {
                                R.send_keys[(u64)o * R.cap + cbase + j] = GS_KEY_INVALID;
                                R.send_idx[(u64)o * R.cap + cbase + j] = 0xffffffffu;
                            }
                        u64 nb = 0;
                        if (lane == 0) nb = atomicAdd(&R.cursors[o], (u64)GS_ROUTE_CHUNK);
                        cbase = ((u64)(uint32_t)gs_rfl((int)(nb >> 32)) << 32) | (uint32_t)gs_rfl((int)nb);
                        used = 0;
                        if (lane == 0) s_base[wv][o] = cbase;
                    }
                    const bool fits = cbase + GS_ROUTE_CHUNK <= R.cap;  // (else: the region is full, the host falls back)
                    if (!fits && lane == 0) R.cursors[64] = 1;
                    if (owner == o && fits) {
                        const u64 at = (u64)o * R.cap + cbase + used + (u64)__popcll(mine & ((1ULL << lane) - 1));
                        R.send_keys[at] = key[s];
                        R.send_idx[at] = (uint32_t)(pb + (u64)p);
                    }
                    if (lane == 0) s_used[wv][o] = used + cnt;
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                    todo &= ~mine;
                }
            }
        }
    }
    // pad the chunks that are still open
    for (int o = 0; o < n_parts; o++) {
        const uint32_t used = s_used[wv][o];
        const u64 cbase = s_base[wv][o];
        if (used < GS_ROUTE_CHUNK && cbase + GS_ROUTE_CHUNK <= R.cap)
            for (uint32_t j = used + (uint32_t)lane; j < GS_ROUTE_CHUNK; j += 64) {
                R.send_keys[(u64)o * R.cap + cbase + j] = GS_KEY_INVALID;
                R.send_idx[(u64)o * R.cap + cbase + j] = 0xffffffffu;
            }
    }
}

// scatter of the answers of one owner region: nodes[idx[i]] = back[i] (sentinel slots skipped)
__global__ __launch_bounds__(256) void gs_unroute_region_kernel(const uint32_t *idx, const int32_t *back, int64_t n, int32_t *nodes) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t at = idx[i];
        if (at != 0xffffffffu) nodes[at] = back[i];
    }
}

extern "C" hipError_t gs_launch_encode_route(const GsEncodeParams *P, const GsRouteParams *R, int grid, hipStream_t stream) {
    if (P->k == 31)
        hipLaunchKernelGGL(gs_encode_route_kernel<31>, dim3(grid), dim3(GS_BLOCK), 0, stream, *P, *R);
    else
        hipLaunchKernelGGL(gs_encode_route_kernel<0>, dim3(grid), dim3(GS_BLOCK), 0, stream, *P, *R);
    return hipGetLastError();
}

extern "C" hipError_t gs_launch_unroute_region(const uint32_t *idx, const int32_t *back, int64_t n, int32_t *nodes, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(gs_unroute_region_kernel, dim3((int)std::min<int64_t>((n + 255) / 256, 256 * 16)), dim3(256), 0, stream, idx, back, n, nodes);
    return hipGetLastError();
}

// ---- routing of the keys to their owner ranks (counting sort by owner; order inside an owner group is arbitrary,
// idx remembers where every routed key came from)
__global__ __launch_bounds__(256) void gs_route_count_kernel(const u64 *keys, int64_t n, int n_parts, u64 *counts) {
    __shared__ unsigned int s_cnt[64];
    const int lane = gs_lane();
    if (threadIdx.x < 64) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t base = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) & ~63LL; base < n; base += stride) {
        const int64_t i = base + lane;
        const u64 h = i < n ? keys[i] : GS_KEY_INVALID;
        const int owner = GS_KEY_ROUTED(h) ? (int)((h >> GS_OWNER_SHIFT) % (u64)n_parts) : -1;
        u64 todo = __ballot(owner >= 0);
        while (todo) {  // one LDS atomic per wave and distinct owner
            const int o = gs_readlane(owner, __builtin_ctzll(todo));
            const u64 mine = __ballot(owner == o);
            if (lane == 0) atomicAdd(&s_cnt[o], (unsigned int)__popcll(mine));
            todo &= ~mine;
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < n_parts && s_cnt[threadIdx.x]) atomicAdd(&counts[threadIdx.x], (u64)s_cnt[threadIdx.x]);
}

// tiles of 4096 keys per workgroup: ranks inside the tile come from LDS counters (one LDS atomic per wave and owner),
// then ONE global atomic per owner and tile reserves the output range -- a single hot cursor would serialise the chip
#define GS_ROUTE_T 16
// nodes (may be NULL): the positions that are not routed get their node here already (miss / invalid window), so that
// gs_unroute_kernel only has to scatter what comes back
__global__ __launch_bounds__(256) void gs_route_scatter_kernel(const u64 *keys, int64_t n, int n_parts, u64 *cursors,
                                                              u64 *send_keys, uint32_t *idx, int32_t *nodes) {
    __shared__ unsigned int s_cnt[64];
    __shared__ u64 s_base[64];
    const int lane = gs_lane();
    const int64_t tile = 256 * GS_ROUTE_T;
    for (int64_t t0 = (int64_t)blockIdx.x * tile; t0 < n; t0 += (int64_t)gridDim.x * tile) {
        if (threadIdx.x < 64) s_cnt[threadIdx.x] = 0;
        __syncthreads();
        u64 h[GS_ROUTE_T];
        int owner[GS_ROUTE_T];
        unsigned int lp[GS_ROUTE_T];
#pragma unroll
        for (int j = 0; j < GS_ROUTE_T; j++) {
            const int64_t i = t0 + (int64_t)j * 256 + threadIdx.x;
            h[j] = i < n ? keys[i] : GS_KEY_INVALID;
            owner[j] = GS_KEY_ROUTED(h[j]) ? (int)((h[j] >> GS_OWNER_SHIFT) % (u64)n_parts) : -1;
            if (nodes != nullptr && i < n && owner[j] < 0) nodes[i] = h[j] == GS_KEY_MISS ? GS_NODE_MISS : GS_NODE_INVALID;
            lp[j] = 0;
            u64 todo = __ballot(owner[j] >= 0);
            while (todo) {
                const int first = __builtin_ctzll(todo);
                const int o = gs_readlane(owner[j], first);
                const u64 mine = __ballot(owner[j] == o);
                unsigned int b = 0;
                if (lane == first) b = atomicAdd(&s_cnt[o], (unsigned int)__popcll(mine));
                b = (unsigned int)gs_readlane((int)b, first);
                if (owner[j] == o) lp[j] = b + (unsigned int)__popcll(mine & ((1ULL << lane) - 1));
                todo &= ~mine;
            }
        }
        __syncthreads();
        if ((int)threadIdx.x < n_parts) s_base[threadIdx.x] = s_cnt[threadIdx.x] ? atomicAdd(&cursors[threadIdx.x], (u64)s_cnt[threadIdx.x]) : 0;
        __syncthreads();
#pragma unroll
        for (int j = 0; j < GS_ROUTE_T; j++) {
            if (owner[j] >= 0) {
                const u64 p = s_base[owner[j]] + lp[j];
                send_keys[p] = h[j];
                idx[p] = (uint32_t)(t0 + (int64_t)j * 256 + threadIdx.x);
            }
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void gs_unroute_kernel(const u64 *keys, const uint32_t *idx, const int32_t *back,
                                                        int64_t n_routed, int32_t *nodes, int64_t n_keys, int phase) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    if (phase == 0)  // positions that were never routed: windows with a bad base, k-mers the gate ruled out
                     // (only when gs_route_scatter_kernel has not written them already)
        for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_keys; i += stride)
            nodes[i] = keys[i] == GS_KEY_MISS ? GS_NODE_MISS : GS_NODE_INVALID;
    else
        for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_routed; i += stride) nodes[idx[i]] = back[i];
}

// one lane per key; marks the slot's seen bit like the fused kernel does
__global__ __launch_bounds__(256) void gs_probe_keys_kernel(GsDbDev db, const u64 *keys, int64_t n, int32_t *nodes,
                                                           int count_unique) {
    const uint32_t vmask2 = 2u * ((1u << db.vbits) - 1u);
    const int shift_rem = (int)db.vbits + 3;
    const uint32_t bmask = (uint32_t)db.bucket_mask;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const u64 h = keys[i];
        int node = h == GS_KEY_MISS ? GS_NODE_MISS : GS_NODE_INVALID;
        if (GS_KEY_ROUTED(h)) {
            node = GS_NODE_MISS;
            bool cand = true;
            if (db.gate != nullptr) {
                const u64 g = gs_gate_bits(h);
                cand = (db.gate[(h >> db.bucket_bits) & db.gate_mask] & g) == g;
            }
            const uint32_t home = (uint32_t)h & bmask;
            const u64 want = (h >> db.bucket_bits) << shift_rem;
            for (int disp = 0; cand && disp <= GS_MAX_DISP; disp++) {
                const uint32_t b = (home + (uint32_t)disp) & bmask;
                GsBucket bk;
                gs_load_bucket(db.table, b, bk);
                int vs = -1, sl = 0;
                const bool done = gs_match_bucket(bk, want | ((u64)disp << (db.vbits + 1)), vmask2, vs, sl);
                if (vs >= 0) {
                    node = vs >> 1;
                    if (count_unique && (vs & 1) == 0)
                        atomicOr(const_cast<u64 *>(db.table) + (size_t)b * GS_SLOTS_PER_BUCKET + sl, 1ULL);
                }
                if (done) break;
            }
        }
        nodes[i] = node;
    }
}

extern "C" hipError_t gs_launch_encode(const GsEncodeParams *P, int grid, hipStream_t stream) {
    if (P->k == 31)
        hipLaunchKernelGGL(gs_encode_kernel<31>, dim3(grid), dim3(GS_BLOCK), 0, stream, *P);
    else
        hipLaunchKernelGGL(gs_encode_kernel<0>, dim3(grid), dim3(GS_BLOCK), 0, stream, *P);
    return hipGetLastError();
}

static int gs_stream_grid(int64_t n) {
    int grid = (int)std::min<int64_t>((n + 255) / 256, 256 * 16);
    return grid < 1 ? 1 : grid;
}

extern "C" hipError_t gs_launch_route_count(const u64 *keys, int64_t n, int n_parts, u64 *counts, hipStream_t stream) {
    hipLaunchKernelGGL(gs_route_count_kernel, dim3(gs_stream_grid(n)), dim3(256), 0, stream, keys, n, n_parts, counts);
    return hipGetLastError();
}

extern "C" hipError_t gs_launch_route_scatter(const u64 *keys, int64_t n, int n_parts, u64 *cursors, u64 *send_keys,
                                               uint32_t *idx, int32_t *nodes, hipStream_t stream) {
    int grid = (int)std::min<int64_t>((n + 256 * GS_ROUTE_T - 1) / (256 * GS_ROUTE_T), 256 * 8);
    if (grid < 1) grid = 1;
    hipLaunchKernelGGL(gs_route_scatter_kernel, dim3(grid), dim3(256), 0, stream, keys, n, n_parts, cursors, send_keys, idx,
                       nodes);
    return hipGetLastError();
}

extern "C" hipError_t gs_launch_unroute(const u64 *keys, const uint32_t *idx, const int32_t *back, int64_t n_routed,
                                         int32_t *nodes, int64_t n_keys, hipStream_t stream) {
    if (keys != nullptr)  // (NULL: gs_route_scatter_kernel has filled in the unrouted positions)
        hipLaunchKernelGGL(gs_unroute_kernel, dim3(gs_stream_grid(n_keys)), dim3(256), 0, stream, keys, idx, back, n_routed,
                           nodes, n_keys, 0);
    if (n_routed > 0)
        hipLaunchKernelGGL(gs_unroute_kernel, dim3(gs_stream_grid(n_routed)), dim3(256), 0, stream, keys, idx, back,
                           n_routed, nodes, n_keys, 1);
    return hipGetLastError();
}

extern "C" hipError_t gs_launch_probe_keys(const GsDbDev *db, const u64 *keys, int64_t n, int32_t *nodes, int count_unique,
                                            hipStream_t stream) {
    int grid = (int)std::min<int64_t>((n + 255) / 256, 256 * 24);
    if (grid < 1) grid = 1;
    hipLaunchKernelGGL(gs_probe_keys_kernel, dim3(grid), dim3(256), 0, stream, *db, keys, n, nodes, count_unique);
    return hipGetLastError();
}
