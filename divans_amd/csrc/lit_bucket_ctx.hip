// lit_bucket_ctx.hip -- bucketed model pass of the ENCODER for context-keyed rows: a context map in use and every reachable mixing
// value 0 -- what host_stream.cpp writes whenever a stream's PredictionMode names no mixing values -- with one model or two and
// any number of literal block types the codec keeps tables for.
//
// With mixing value 0 (codec/literal.rs:176-208, mm_opts == 0) a position's high nibble is coded with row high[0][0][ctx] and its low
// nibble with row low[0][ctx][hi]; with dynamic mixing the context-map model adds First[ctx] and Second[hi][ctx].  Every row a
// position touches is a function of ctx ALONE: 1 high row + 16 low rows per key and model -- the bucket of bucket_chain_kernel and of
// mix_chain_kernel<1>.  So ONE sort by ctx serves both models (one task list, one inv), and what is new is the key:
//   ctx(p) = LIT_BLOB_CTXF[bt(p) - bt_first][prev(p)][lut1 class of prev_prev(p)]
// where bt(p) is the block type of the segment that covers p.  Everything behind the sort is the code of the other two passes:
//   one model   bucket_tasks_kernel, bucket_chain_kernel (literal_adaptation[0]), bucket_unsort_kernel                 (lit_bucket.hip)
//   two models  bucket_tasks_kernel once, then two chain launches over the same task list -- mix_chain_ctx_kernel<0> (both nibbles
//               literal_adaptation[0], planes 0) and mix_chain_kernel<1> (planes 1) --, the four unsorts through the shared inv,
//               mix_weights_kernel                                                                                      (lit_bucket_mix.hip)
#include "lit_bucket_dev.h"

namespace divans_hip {

// marks of the SEG instances, one byte per position of the piece (in `staging`, which is free until placement)
constexpr uint32_t CX_BT = 15u;          // bits 0..3: table + 1 of the segment that starts here (or covers the piece base), 0 = none
constexpr uint32_t CX_KEYED = 0xc0u;     // bit 7: first position of a segment, bit 6: its second -- the walk has formed the key already

// ---------------------------------------------------------------------------------------------
// per (stream, piece): sorted[slot] = byte (PAY16: in 16 bits, what the two-model chains load), inv[pos] = slot,
// desc[stream][ctx][piece] = start | count << 16.  The ranking, scan and placement are bucket_sort_kernel's (one ranking pass over
// LDS lane masks, lit_bucket.hip).
// SEG = false: every position has the configuration's own block type (table 0 of the blob, staged in LDS) and the history is the
//   bytes before it (zero before the stream): keys are formed where they are needed, nothing else is kept.  22.8 KB of LDS: seven
//   workgroups per CU.
// SEG = true: the workgroup walks the stream's list once (bk_seg_walk).  The lane that holds a non-empty segment
//   - marks table + 1 at the segment's first position, or at the piece base when the segment starts before the piece and covers it,
//   - forms the keys of the segment's first two positions itself (it knows their block type: its own): prev / prev_prev from last8
//     as in mix_sort_kernel<1, true>; a one-byte segment leaves its second position to the segment that follows.
//   Then "last mark at or before p" is propagated -- every lane takes 32 consecutive positions, the 256 carries meet in one scan --
//   and the remaining keys are formed with the table found (none: table 0).  A block type outside the tables takes table 0 (the
//   walk of piece 0 reports it).  The tables (up to 16 KB) are read from the blob in global memory, once per position; the keys stay
//   in LDS (8 KB): 28.9 KB, five workgroups per CU as bucket_sort_kernel<true>.
// ---------------------------------------------------------------------------------------------
template <bool PAY16, bool SEG>
__global__ __launch_bounds__(BK_SORT_THREADS) void ctx_sort_kernel(const MixBucketBatch b) {
    __shared__ __attribute__((aligned(16))) unsigned long long staging64[BK_PIECE / 8u];   // SEG: marks; lane masks while ranking; then the sorted bytes
    uint8_t* staging = (uint8_t*)staging64;
    __shared__ __attribute__((aligned(16))) uint8_t piece_in[16 + BK_PIECE];   // piece_in[14], [15] = the two bytes before the piece
    __shared__ uint32_t hist[4][256];
    __shared__ uint32_t wsum[4];
    __shared__ uint8_t lut1c[256];
    __shared__ __attribute__((aligned(4))) uint8_t ctxf[SEG ? 4u : LIT_CTXF_BYTES];   // !SEG: the one table
    __shared__ uint8_t kp[SEG ? BK_PIECE : 1u];                                       // SEG: the key of every position
    const uint32_t s = blockIdx.x / b.pieces, piece = blockIdx.x % b.pieces;
    const uint32_t tid = threadIdx.x, w = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6)), lane = tid & 63;
    const uint32_t len = b.in_sizes ? b.in_sizes[s] : b.stream_len;
    const uint8_t* in = b.in + (b.in_offsets ? b.in_offsets[s] : (uint64_t)s * b.stream_len);
    uint32_t* desc = b.desc + ((size_t)s * 256u + tid) * 8u + piece;
    const uint32_t base = piece * BK_PIECE;
    if (base >= len) {
        *desc = 0u;
        if (SEG && piece == 0u)     // an empty stream: its list still has to add up to it
            bk_seg_walk(b.seg_begin, b.segs, s, 0u, ~0u, true, b.bt_first, b.n_btypes, b.status, wsum, [](uint32_t, uint32_t, uint64_t) {});
        return;
    }
    const uint32_t n = len - base < BK_PIECE ? len - base : BK_PIECE;
    const size_t pl = b.slot;
    for (uint32_t i = tid; i < 1024u; i += BK_SORT_THREADS) (&hist[0][0])[i] = 0u;
    lut1c[tid] = b.blob[LIT_BLOB_LUT1CLASS + tid] & 7u;
    if (!SEG) for (uint32_t i = tid; i < LIT_CTXF_BYTES / 4u; i += BK_SORT_THREADS) ((uint32_t*)ctxf)[i] = ((const uint32_t*)(b.blob + LIT_BLOB_CTXF))[i];
    if (SEG) for (uint32_t i = tid; i < BK_PIECE / 16u; i += BK_SORT_THREADS) ((u32x4*)staging)[i] = u32x4{0u, 0u, 0u, 0u};
    bk_load_piece(piece_in, in + base, n);
    if (tid == 0u) { piece_in[15] = base ? in[base - 1u] : 0u; piece_in[14] = base ? in[base - 2u] : 0u; }   // last_8_literals starts at zero
    __syncthreads();
    if (SEG) {
        const uint8_t* tables = b.blob + LIT_BLOB_CTXF;
        const auto key_of = [&](uint32_t table, uint32_t prev, uint32_t prev_prev) -> uint8_t {      // table < n_btypes <= LIT_MAX_BTYPES
            return tables[table * LIT_CTXF_BYTES + (prev << 3) + lut1c[prev_prev]];
        };
        const uint32_t bt_first = b.bt_first, n_btypes = b.n_btypes;
        // every position (mark and key) is written by one lane at most: non-empty segments do not overlap
        bk_seg_walk(b.seg_begin, b.segs, s, len, piece == 0u ? ~0u : base + n, piece == 0u, bt_first, n_btypes, b.status, wsum,
                    [&](uint32_t q, uint32_t l, uint64_t l8, uint32_t btype) {
                        const uint32_t table = btype - bt_first < n_btypes ? btype - bt_first : 0u;
                        const uint32_t newest = (uint32_t)(l8 >> 56), before = (uint32_t)(l8 >> 48) & 0xffu;
                        const uint32_t p = q - base, p1 = q + 1u - base;
                        if (p < n) { kp[p] = key_of(table, newest, before); staging[p] = (uint8_t)(0x80u | (table + 1u)); }
                        else if (q < base && q + l > base) staging[0] = (uint8_t)((table + 1u) | (p1 == 0u ? 0x40u : 0u));   // covers the base (p1 == 0: l >= 2)
                        if (l >= 2u && p1 < n) {
                            kp[p1] = key_of(table, piece_in[15u + p1], newest);
                            if (p1 != 0u) staging[p1] = 0x40u;
                        }
                    });
        __syncthreads();
        // the last mark at or before every position: lane tid owns positions [32 tid, 32 tid + 32)
        {
            u32x4* mine = (u32x4*)staging + 2u * tid;
            const u32x4 m0 = mine[0], m1 = mine[1];
            uint32_t wd[8] = {m0.x, m0.y, m0.z, m0.w, m1.x, m1.y, m1.z, m1.w};
            uint32_t last = 0u;
#pragma unroll
            for (uint32_t j = 0; j < 8u; ++j)
#pragma unroll
                for (uint32_t k = 0; k < 4u; ++k) { const uint32_t v = (wd[j] >> (8u * k)) & CX_BT; if (v) last = v; }
            uint32_t incl = last;       // inclusive scan under (a, b) -> b ? b : a
            for (uint32_t d = 1; d < 64u; d <<= 1) {
                const uint32_t v = (uint32_t)__shfl_up((int)incl, d, 64);
                if (lane >= d && incl == 0u) incl = v;
            }
            if (lane == 63u) wsum[w] = incl;
            __syncthreads();
            uint32_t cur = (uint32_t)__shfl_up((int)incl, 1, 64);
            if (lane == 0u) cur = 0u;
            for (uint32_t j = 3u; j-- > 0u;) if (j < w && cur == 0u) cur = wsum[j];
#pragma unroll
            for (uint32_t j = 0; j < 8u; ++j) {
                uint32_t o = 0u;
#pragma unroll
                for (uint32_t k = 0; k < 4u; ++k) {
                    const uint32_t m = (wd[j] >> (8u * k)) & 0xffu;
                    if (m & CX_BT) cur = m & CX_BT;
                    o |= ((m & CX_KEYED) | cur) << (8u * k);
                }
                wd[j] = o;
            }
            mine[0] = u32x4{wd[0], wd[1], wd[2], wd[3]}; mine[1] = u32x4{wd[4], wd[5], wd[6], wd[7]};
        }
        __syncthreads();
        for (uint32_t bt = 0; bt < 32u; ++bt) {
            const uint32_t p = w * 2048u + bt * 64u + lane;
            if (p < n) {
                const uint32_t m = staging[p];
                if (!(m & CX_KEYED)) kp[p] = key_of((m & CX_BT) ? (m & CX_BT) - 1u : 0u, piece_in[15u + p], piece_in[14u + p]);
            }
        }
        __syncthreads();
    }
    const auto key_at = [&](uint32_t p) -> uint32_t {
        return SEG ? (uint32_t)kp[p] : (uint32_t)ctxf[((uint32_t)piece_in[15u + p] << 3) + lut1c[piece_in[14u + p]]];
    };
    // ONE ranking pass, as in bucket_sort_kernel (where it is explained): wave w owns positions [2048 w, 2048 w + 2048)
    unsigned long long* mask_of = staging64 + w * 256u;     // relaxed atomics below: lanes meet in these words, nothing may be forwarded
    const unsigned long long my_bit = 1ull << lane;
    uint32_t kept[16];
#pragma unroll
    for (uint32_t bt = 0; bt < 32u; ++bt) {
        uint32_t r = 0;
        const uint32_t p = w * 2048u + bt * 64u + lane;
        if (p < n) {
            const uint32_t key = key_at(p);
            __hip_atomic_store(mask_of + key, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            __hip_atomic_fetch_or(mask_of + key, my_bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            const unsigned long long same = __hip_atomic_load(mask_of + key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            const uint32_t rank = lanes_below(same), cnt = (uint32_t)__popcll(same);
            const uint32_t before = hist[w][key];
            r = before + rank;
            if (rank == cnt - 1u) hist[w][key] = before + cnt;
        }
        if (bt & 1u) kept[bt >> 1] |= r << 16; else kept[bt >> 1] = r;
    }
    __syncthreads();
    // the 256 totals' exclusive scan: each wave scans its 64 keys with shuffles, the four wave sums meet in LDS
    const uint32_t c0 = hist[0][tid], c1 = hist[1][tid], c2 = hist[2][tid], c3 = hist[3][tid];
    const uint32_t tot = c0 + c1 + c2 + c3;
    uint32_t incl = tot;
    for (uint32_t d = 1; d < 64u; d <<= 1) {
        const uint32_t v = (uint32_t)__shfl_up((int)incl, d, 64);
        if (lane >= d) incl += v;
    }
    if (lane == 63u) wsum[w] = incl;
    __syncthreads();
    uint32_t start = incl - tot;
    for (uint32_t j = 0; j < 3u; ++j) if (j < w) start += wsum[j];
    hist[0][tid] = start; hist[1][tid] = start + c0; hist[2][tid] = start + c0 + c1; hist[3][tid] = start + c0 + c1 + c2;
    *desc = start | (tot << 16);
    __syncthreads();
    // placement: the slot is the key's base for this wave + the kept rank
    uint16_t* inv = b.inv + (size_t)s * pl + base;
#pragma unroll
    for (uint32_t bt = 0; bt < 32u; ++bt) {
        const uint32_t p = w * 2048u + bt * 64u + lane;
        if (p < n) {
            const uint32_t key = key_at(p), byte = piece_in[16u + p];
            const uint32_t slot = hist[w][key] + ((kept[bt >> 1] >> (16u * (bt & 1u))) & 0xffffu);
            staging[slot] = (uint8_t)byte;
            inv[p] = (uint16_t)slot;
        }
    }
    __syncthreads();
    if (PAY16) {
        uint16_t* sorted = b.sorted + (size_t)s * pl + base;
        for (uint32_t i = tid * 8u; i < n; i += BK_SORT_THREADS * 8u) {
            if (i + 8u <= n) {
                const u32x2 v = *(const u32x2*)(staging + i);
                const u32x4 o = {(v.x & 0xffu) | ((v.x & 0xff00u) << 8), ((v.x >> 16) & 0xffu) | ((v.x >> 24) << 16),
                                 (v.y & 0xffu) | ((v.y & 0xff00u) << 8), ((v.y >> 16) & 0xffu) | ((v.y >> 24) << 16)};
                *(u32x4*)(sorted + i) = o;
            } else for (uint32_t k = i; k < n; ++k) sorted[k] = staging[k];
        }
    } else {
        uint8_t* sorted = (uint8_t*)b.sorted + (size_t)s * pl + base;
        for (uint32_t i = tid * 16u; i < n; i += BK_SORT_THREADS * 16u) {
            if (i + 16u <= n) *(u32x4*)(sorted + i) = *(const u32x4*)(staging + i);
            else for (uint32_t k = i; k < n; ++k) sorted[k] = staging[k];
        }
    }
}

template <bool PAY16>
static hipError_t ctx_prepare_and_sort(const MixBucketBatch& b, hipStream_t st) {
    hipError_t e = hipMemsetAsync(b.counters, 0, 64, st);
    if (e != hipSuccess) return e;
    if (b.pieces < 8u) {
        e = hipMemsetAsync(b.desc, 0, (size_t)b.n_streams * 256u * 8u * sizeof(uint32_t), st);
        if (e != hipSuccess) return e;
    }
    if (b.segs) hipLaunchKernelGGL((ctx_sort_kernel<PAY16, true>), dim3(b.n_streams * b.pieces), dim3(BK_SORT_THREADS), 0, st, b);
    else hipLaunchKernelGGL((ctx_sort_kernel<PAY16, false>), dim3(b.n_streams * b.pieces), dim3(BK_SORT_THREADS), 0, st, b);
    return hipGetLastError();
}

// the view the task-list and unsort kernels (and, with one model, the chain kernel) take
static BucketBatch ctx_view(const MixBucketBatch& b) {
    BucketBatch v;
    v.in = b.in; v.in_offsets = b.in_offsets; v.in_sizes = b.in_sizes;
    v.n_streams = b.n_streams; v.stream_len = b.stream_len; v.max_stream_len = b.max_stream_len; v.pieces = b.pieces;
    v.slot = b.slot; v.sf_stride = 2u * b.pos_stride;
    v.sorted = (uint8_t*)b.sorted; v.inv = b.inv; v.desc = b.desc; v.sfs = nullptr; v.sf = nullptr; v.tasks = b.tasks; v.counters = b.counters;
    v.inc = b.inc0; v.lim = b.lim0;
    v.seg_begin = nullptr; v.segs = nullptr; v.bt_first = 0; v.n_btypes = 0; v.status = nullptr;   // (the sort kernels here take `b`)
    return v;
}

// one model: b.sorted holds bytes, b.xs[0] = where the pairs go (sorted order, then position order in place; pos_stride == slot)
hipError_t launch_bucket_ctx_model(const MixBucketBatch& b, uint32_t chain_blocks, hipStream_t st) {
    hipError_t e = ctx_prepare_and_sort<false>(b, st);
    if (e != hipSuccess) return e;
    BucketBatch v = ctx_view(b);
    v.sfs = b.xs[0]; v.sf = (uint32_t*)b.xs[0];
    launch_bucket_tasks(v, st);
    launch_bucket_chain(v, chain_blocks, st);
    launch_bucket_unsort(v, st);
    return hipGetLastError();
}

hipError_t launch_bucket_ctx_mix_model(const MixBucketBatch& b, uint32_t num_cus, hipStream_t st) {
    hipError_t e = ctx_prepare_and_sort<true>(b, st);
    if (e != hipSuccess) return e;
    BucketBatch v = ctx_view(b);
    launch_bucket_tasks(v, st);
    for (int model = 0; model < 2; ++model) {
        if (model == 1) {       // the second chain launch hands the same task list out again
            e = hipMemsetAsync(b.counters + BK_CLAIM, 0, sizeof(uint32_t), st);
            if (e != hipSuccess) return e;
        }
        launch_mix_chain_ctx(b, model, num_cus, st);
    }
    for (int model = 0; model < 2; ++model) {
        v.sfs = b.xs[model]; v.sf = (uint32_t*)b.xs[model]; v.sf_stride = 2u * b.pos_stride;
        launch_bucket_unsort(v, st);
        v.sfs = (bk_u32x2*)b.maxes[model]; v.sf = b.maxes[model]; v.sf_stride = b.pos_stride;
        launch_bucket_unsort32(v, st);
    }
    launch_mix_weights(b, num_cus, st);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// Several block types under mixing value 4 with two models (launch_bucket_mix_bt_model).  The stride model's rows are high
// [ctx][prev] and low [prev][hi] (literal.rs:205-208): its buckets stay keyed by prev as in mix_sort_kernel<0, .>, and the block type
// only helps to pick the HIGH row -- ctx = LIT_BLOB_CTXF[bt][prev][class of prev_prev] -- so it enters the payload's high-row slot
// (bits 8..10, what mix_chain_kernel<0> indexes its eight high rows with), not the key.  The slot is the index of ctx among the
// contexts prev reaches over all block types; the host numbers them (derive_high_row_slots, capi.cpp: at most eight, or the pass
// is refused) into tables laid out like the context tables, behind the mixing mask of the blob.
//
// mix_bt_sort_kernel, per (stream, piece): sorted[slot position] = byte | high-row slot << 8, inv[pos], desc[stream][prev][piece].
// Ranking, scan and placement are ctx_sort_kernel's; a rank stays below 2112 (2048 positions of the wave + 64), so the slot rides
// in bits 13..15 of the kept rank and the slot array is free again at placement, where it receives the slots in sorted order.
// SEG = false: one table (table 0 of the blob, the one ctx_sort_kernel<., false> takes for such a call), staged in LDS; key and
//   slot are formed where they are needed.  LDS 30.3 KB: five workgroups per CU; 50 VGPRs.
// SEG = true: the walk, the marks and the "last mark at or before p" scan of ctx_sort_kernel<., true>.  The lane that holds a
//   segment forms key and slot of its first position (prev / prev_prev = the two newest bytes of last8) and the slot of its second
//   (prev_prev = last8's newest) under its own block type; every other position takes the table found (none, or a block type
//   outside the tables: table 0 -- piece 0's walk reports those and lists that do not add up).  The slot tables (up to 16 KB) are
//   read from global memory, once per position.  Kept per position: key and slot, one byte array each -- with the marks / lane
//   masks / sorted bytes (8 KB), the piece (8 KB) and the counts (4 KB) 36.3 KB of LDS: four workgroups per CU (mix_sort_kernel<0,
//   true>, with 16-bit staging and 16-bit kp, has three); 79 VGPRs.
// ---------------------------------------------------------------------------------------------
template <bool SEG>
__global__ __launch_bounds__(BK_SORT_THREADS) void mix_bt_sort_kernel(const MixBucketBatch b) {
    __shared__ __attribute__((aligned(16))) unsigned long long staging64[BK_PIECE / 8u];   // SEG: marks; lane masks while ranking; then the sorted bytes
    uint8_t* staging = (uint8_t*)staging64;
    __shared__ __attribute__((aligned(16))) uint8_t piece_in[16 + BK_PIECE];   // piece_in[14], [15] = the two bytes before the piece
    __shared__ __attribute__((aligned(16))) uint8_t sl[BK_PIECE];              // SEG: the slot of every position until ranking; then the slots in sorted order
    __shared__ uint32_t hist[4][256];
    __shared__ uint32_t wsum[4];
    __shared__ uint8_t lut1c[256];
    __shared__ __attribute__((aligned(4))) uint8_t slot0[SEG ? 4u : LIT_CTXF_BYTES];   // !SEG: the one slot table
    __shared__ uint8_t kp[SEG ? BK_PIECE : 1u];                                        // SEG: the key of every position
    const uint32_t s = blockIdx.x / b.pieces, piece = blockIdx.x % b.pieces;
    const uint32_t tid = threadIdx.x, w = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6)), lane = tid & 63;
    const uint32_t len = b.in_sizes ? b.in_sizes[s] : b.stream_len;
    const uint8_t* in = b.in + (b.in_offsets ? b.in_offsets[s] : (uint64_t)s * b.stream_len);
    uint32_t* desc = b.desc + ((size_t)s * 256u + tid) * 8u + piece;
    const uint32_t base = piece * BK_PIECE;
    if (base >= len) {
        *desc = 0u;
        if (SEG && piece == 0u)     // an empty stream: its list still has to add up to it
            bk_seg_walk(b.seg_begin, b.segs, s, 0u, ~0u, true, b.bt_first, b.n_btypes, b.status, wsum, [](uint32_t, uint32_t, uint64_t) {});
        return;
    }
    const uint32_t n = len - base < BK_PIECE ? len - base : BK_PIECE;
    const size_t pl = b.slot;
    const uint8_t* tables = b.blob + LIT_BLOB_CTXF + LIT_CTXF_BYTES * b.n_btypes + 8192u;    // slot_of[block type][prev][class], behind the mixing mask
    for (uint32_t i = tid; i < 1024u; i += BK_SORT_THREADS) (&hist[0][0])[i] = 0u;
    lut1c[tid] = b.blob[LIT_BLOB_LUT1CLASS + tid] & 7u;
    if (!SEG) for (uint32_t i = tid; i < LIT_CTXF_BYTES / 4u; i += BK_SORT_THREADS) ((uint32_t*)slot0)[i] = ((const uint32_t*)tables)[i];
    if (SEG) for (uint32_t i = tid; i < BK_PIECE / 16u; i += BK_SORT_THREADS) ((u32x4*)staging)[i] = u32x4{0u, 0u, 0u, 0u};
    bk_load_piece(piece_in, in + base, n);
    if (tid == 0u) { piece_in[15] = base ? in[base - 1u] : 0u; piece_in[14] = base ? in[base - 2u] : 0u; }   // last_8_literals starts at zero
    __syncthreads();
    if (SEG) {
        const auto slot_of = [&](uint32_t table, uint32_t prev, uint32_t prev_prev) -> uint8_t {      // table < n_btypes <= LIT_MAX_BTYPES; < 8 (the host refuses more)
            return tables[table * LIT_CTXF_BYTES + (prev << 3) + lut1c[prev_prev]] & 7u;
        };
        const uint32_t bt_first = b.bt_first, n_btypes = b.n_btypes;
        // every position (mark, key and slot) is written by one lane at most: non-empty segments do not overlap
        bk_seg_walk(b.seg_begin, b.segs, s, len, piece == 0u ? ~0u : base + n, piece == 0u, bt_first, n_btypes, b.status, wsum,
                    [&](uint32_t q, uint32_t l, uint64_t l8, uint32_t btype) {
                        const uint32_t table = btype - bt_first < n_btypes ? btype - bt_first : 0u;
                        const uint32_t newest = (uint32_t)(l8 >> 56), before = (uint32_t)(l8 >> 48) & 0xffu;
                        const uint32_t p = q - base, p1 = q + 1u - base;
                        if (p < n) { kp[p] = (uint8_t)newest; sl[p] = slot_of(table, newest, before); staging[p] = (uint8_t)(0x80u | (table + 1u)); }
                        else if (q < base && q + l > base) staging[0] = (uint8_t)((table + 1u) | (p1 == 0u ? 0x40u : 0u));   // covers the base (p1 == 0: l >= 2)
                        if (l >= 2u && p1 < n) {
                            const uint32_t prev = piece_in[15u + p1];
                            kp[p1] = (uint8_t)prev; sl[p1] = slot_of(table, prev, newest);
                            if (p1 != 0u) staging[p1] = 0x40u;
                        }
                    });
        __syncthreads();
        // the last mark at or before every position: lane tid owns positions [32 tid, 32 tid + 32)
        {
            u32x4* mine = (u32x4*)staging + 2u * tid;
            const u32x4 m0 = mine[0], m1 = mine[1];
            uint32_t wd[8] = {m0.x, m0.y, m0.z, m0.w, m1.x, m1.y, m1.z, m1.w};
            uint32_t last = 0u;
#pragma unroll
            for (uint32_t j = 0; j < 8u; ++j)
#pragma unroll
                for (uint32_t k = 0; k < 4u; ++k) { const uint32_t v = (wd[j] >> (8u * k)) & CX_BT; if (v) last = v; }
            uint32_t incl = last;       // inclusive scan under (a, b) -> b ? b : a
            for (uint32_t d = 1; d < 64u; d <<= 1) {
                const uint32_t v = (uint32_t)__shfl_up((int)incl, d, 64);
                if (lane >= d && incl == 0u) incl = v;
            }
            if (lane == 63u) wsum[w] = incl;
            __syncthreads();
            uint32_t cur = (uint32_t)__shfl_up((int)incl, 1, 64);
            if (lane == 0u) cur = 0u;
            for (uint32_t j = 3u; j-- > 0u;) if (j < w && cur == 0u) cur = wsum[j];
#pragma unroll
            for (uint32_t j = 0; j < 8u; ++j) {
                uint32_t o = 0u;
#pragma unroll
                for (uint32_t k = 0; k < 4u; ++k) {
                    const uint32_t m = (wd[j] >> (8u * k)) & 0xffu;
                    if (m & CX_BT) cur = m & CX_BT;
                    o |= ((m & CX_KEYED) | cur) << (8u * k);
                }
                wd[j] = o;
            }
            mine[0] = u32x4{wd[0], wd[1], wd[2], wd[3]}; mine[1] = u32x4{wd[4], wd[5], wd[6], wd[7]};
        }
        __syncthreads();
        for (uint32_t bt = 0; bt < 32u; ++bt) {
            const uint32_t p = w * 2048u + bt * 64u + lane;
            if (p < n) {
                const uint32_t m = staging[p];
                if (!(m & CX_KEYED)) {
                    const uint32_t prev = piece_in[15u + p];
                    kp[p] = (uint8_t)prev; sl[p] = slot_of((m & CX_BT) ? (m & CX_BT) - 1u : 0u, prev, piece_in[14u + p]);
                }
            }
        }
        __syncthreads();
    }
    const auto key_at = [&](uint32_t p) -> uint32_t { return SEG ? (uint32_t)kp[p] : (uint32_t)piece_in[15u + p]; };
    const auto slot_at = [&](uint32_t p) -> uint32_t {
        return SEG ? (uint32_t)sl[p] : (uint32_t)slot0[((uint32_t)piece_in[15u + p] << 3) + lut1c[piece_in[14u + p]]] & 7u;
    };
    // ONE ranking pass, as in bucket_sort_kernel (where it is explained): wave w owns positions [2048 w, 2048 w + 2048)
    unsigned long long* mask_of = staging64 + w * 256u;     // relaxed atomics below: lanes meet in these words, nothing may be forwarded
    const unsigned long long my_bit = 1ull << lane;
    uint32_t kept[16];      // per position: rank among the wave's positions of its key (< 2112) | slot << 13
#pragma unroll
    for (uint32_t bt = 0; bt < 32u; ++bt) {
        uint32_t r = 0;
        const uint32_t p = w * 2048u + bt * 64u + lane;
        if (p < n) {
            const uint32_t key = key_at(p);
            __hip_atomic_store(mask_of + key, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            __hip_atomic_fetch_or(mask_of + key, my_bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            const unsigned long long same = __hip_atomic_load(mask_of + key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            const uint32_t rank = lanes_below(same), cnt = (uint32_t)__popcll(same);
            const uint32_t before = hist[w][key];
            r = (before + rank) | (slot_at(p) << 13);
            if (rank == cnt - 1u) hist[w][key] = before + cnt;
        }
        if (bt & 1u) kept[bt >> 1] |= r << 16; else kept[bt >> 1] = r;
    }
    __syncthreads();
    // the 256 totals' exclusive scan: each wave scans its 64 keys with shuffles, the four wave sums meet in LDS
    const uint32_t c0 = hist[0][tid], c1 = hist[1][tid], c2 = hist[2][tid], c3 = hist[3][tid];
    const uint32_t tot = c0 + c1 + c2 + c3;
    uint32_t incl = tot;
    for (uint32_t d = 1; d < 64u; d <<= 1) {
        const uint32_t v = (uint32_t)__shfl_up((int)incl, d, 64);
        if (lane >= d) incl += v;
    }
    if (lane == 63u) wsum[w] = incl;
    __syncthreads();
    uint32_t start = incl - tot;
    for (uint32_t j = 0; j < 3u; ++j) if (j < w) start += wsum[j];
    hist[0][tid] = start; hist[1][tid] = start + c0; hist[2][tid] = start + c0 + c1; hist[3][tid] = start + c0 + c1 + c2;
    *desc = start | (tot << 16);
    __syncthreads();
    // placement: the slot position is the key's base for this wave + the kept rank; byte and high-row slot go to their own planes
    uint16_t* inv = b.inv + (size_t)s * pl + base;
#pragma unroll
    for (uint32_t bt = 0; bt < 32u; ++bt) {
        const uint32_t p = w * 2048u + bt * 64u + lane;
        if (p < n) {
            const uint32_t key = key_at(p), byte = piece_in[16u + p];
            const uint32_t kr = (kept[bt >> 1] >> (16u * (bt & 1u))) & 0xffffu;
            const uint32_t at = hist[w][key] + (kr & 0x1fffu);
            staging[at] = (uint8_t)byte;
            sl[at] = (uint8_t)(kr >> 13);
            inv[p] = (uint16_t)at;
        }
    }
    __syncthreads();
    uint16_t* sorted = b.sorted + (size_t)s * pl + base;
    const auto pair_of = [](uint32_t bytes, uint32_t slots) -> uint32_t {      // the low two bytes of each, interleaved
        return (bytes & 0xffu) | ((slots & 0xffu) << 8) | ((bytes & 0xff00u) << 8) | ((slots & 0xff00u) << 16);
    };
    for (uint32_t i = tid * 8u; i < n; i += BK_SORT_THREADS * 8u) {
        if (i + 8u <= n) {
            const u32x2 v = *(const u32x2*)(staging + i), t = *(const u32x2*)(sl + i);
            const u32x4 o = {pair_of(v.x, t.x), pair_of(v.x >> 16, t.x >> 16), pair_of(v.y, t.y), pair_of(v.y >> 16, t.y >> 16)};
            *(u32x4*)(sorted + i) = o;
        } else for (uint32_t k = i; k < n; ++k) sorted[k] = (uint16_t)(staging[k] | ((uint32_t)sl[k] << 8));
    }
}

// The sequence of launch_bucket_mix_model with the two sorts that know block types: mix_bt_sort_kernel for the stride model,
// ctx_sort_kernel<true, .> (16-bit payloads that hold the byte alone: slot 0, the context model's one high row) for the context model.
// (A template -- 0 is the one instance -- so that the sorts it names are instantiated behind those of ctx_prepare_and_sort: the kernels of
// the context-keyed passes keep their places in the code object.)
template <int>
static hipError_t mix_bt_launch(const MixBucketBatch& b, uint32_t num_cus, hipStream_t st) {
    BucketBatch v = ctx_view(b);
    for (int model = 0; model < 2; ++model) {
        hipError_t e = hipMemsetAsync(b.counters, 0, 64, st);
        if (e != hipSuccess) return e;
        if (b.pieces < 8u) {
            e = hipMemsetAsync(b.desc, 0, (size_t)b.n_streams * 256u * 8u * sizeof(uint32_t), st);
            if (e != hipSuccess) return e;
        }
        const dim3 grid(b.n_streams * b.pieces), block(BK_SORT_THREADS);
        if (model == 0) {
            if (b.segs) hipLaunchKernelGGL((mix_bt_sort_kernel<true>), grid, block, 0, st, b);
            else hipLaunchKernelGGL((mix_bt_sort_kernel<false>), grid, block, 0, st, b);
        } else {
            if (b.segs) hipLaunchKernelGGL((ctx_sort_kernel<true, true>), grid, block, 0, st, b);
            else hipLaunchKernelGGL((ctx_sort_kernel<true, false>), grid, block, 0, st, b);
        }
        launch_bucket_tasks(v, st);
        launch_mix_chain(b, model, num_cus, st);
        v.sfs = b.xs[model]; v.sf = (uint32_t*)b.xs[model]; v.sf_stride = 2u * b.pos_stride;
        launch_bucket_unsort(v, st);
        v.sfs = (bk_u32x2*)b.maxes[model]; v.sf = b.maxes[model]; v.sf_stride = b.pos_stride;
        launch_bucket_unsort32(v, st);
    }
    launch_mix_weights(b, num_cus, st);
    return hipGetLastError();
}

hipError_t launch_bucket_mix_bt_model(const MixBucketBatch& b, uint32_t num_cus, hipStream_t st) { return mix_bt_launch<0>(b, num_cus, st); }

}  // namespace divans_hip
