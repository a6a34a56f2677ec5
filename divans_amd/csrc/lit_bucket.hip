// lit_bucket.hip -- bucketed model pass of the ENCODER for the order-1, context-map-off configuration
// (mixing value 4 everywhere, constant context: BASELINE configs[1], reference TestSimple, bin/benchmark.rs:195-206).
//
// In that configuration the high nibble of byte i is coded with row [prev] and its low nibble with row [prev][hi]
// (codec/literal.rs:176-208 with mm_opts == 4), both blended with literal_adaptation[0] (literal.rs:320,354).  A row's
// CDF therefore only depends on the earlier positions that share its `prev` byte.  The encoder knows every byte
// up front, so instead of walking the stream serially against a 139 KB table in HBM (lit_model_encode_kernel) it
//   1. bucket_sort_kernel    stable counting sort of every 8 KiB piece of a stream by prev byte (LDS),
//   2. bucket_tasks_kernel   turns the non-empty (stream, prev) buckets into a task list, longest first,
//   3. bucket_chain_kernel   ONE LANE per bucket walks its positions in order with the bucket's 17 rows
//                            (1 high + 16 low) in LDS -- no table in HBM, no row cache, no cross-lane traffic (the loop
//                            is explained at bk_chain_loop, lit_bucket_dev.h, which the two-model pass runs),
//   4. bucket_unsort_kernel  puts the (start,freq) pairs back into position order for the rANS pass.
// The strides 2, 3, 4 and 8 (every reachable mixing value 5, 6, 7, or 8 and above; constant context) run the same pass: there the
// high row is [ctx][b_d] and the low row [b_d][hi] with b_d the byte d places back (literal.rs:192-208), so only step 1 differs --
// bucket_sort_stride_kernel keys a position by that byte (launch_bucket_stride_model); steps 2-4 never look at what the key was.
// The arithmetic per nibble is the same as everywhere else (probability/interface.rs:97-108, frequentist_cdf.rs:74-85).
// The decoder cannot do this (it learns the bytes one at a time) and keeps the streaming kernels.
#include "lit_bucket_dev.h"

#ifndef DIVANS_BK_CHAIN_NO_STORES   // counterfactual: bucket_chain_kernel keeps its arithmetic and drops its pair stores (WRONG output: timing only)
#define DIVANS_BK_CHAIN_NO_STORES 0
#endif

namespace divans_hip {

// ---------------------------------------------------------------------------------------------
// 1. per (stream, piece): sorted[slot] = byte, inv[pos] = slot, desc[stream][prev][piece] = start | count << 16
//    SEG: the stream has a segment list (b.seg_begin / b.segs): the first byte of every non-empty segment takes its key from the
//    segment's last8 instead of the byte before it (SegCursor, lit_device.h), through an LDS copy of the keys that the workgroup
//    patches while it walks the list (bk_seg_walk); the workgroup of piece 0 checks the list.  SEG = false is the code it was.
// ---------------------------------------------------------------------------------------------
template <bool SEG>
__global__ __launch_bounds__(BK_SORT_THREADS) void bucket_sort_kernel(const BucketBatch b) {
    __shared__ __attribute__((aligned(16))) unsigned long long staging64[BK_PIECE / 8u];   // lane masks while ranking, then the sorted bytes
    uint8_t* staging = (uint8_t*)staging64;
    __shared__ __attribute__((aligned(16))) uint8_t piece_in[16 + BK_PIECE];   // piece_in[15] = the byte before the piece
    __shared__ uint32_t hist[4][256];
    __shared__ uint32_t wsum[4];
    __shared__ uint8_t prev_of[SEG ? BK_PIECE : 1u];     // SEG: the key of every position
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
    // the piece (and the byte before it: the first key) once into LDS
    bk_load_piece(piece_in, in + base, n);
    if (tid == 0u) piece_in[15] = base ? in[base - 1u] : 0u;
    __syncthreads();
    const uint8_t* key_of = piece_in + 15;      // key_of[p] = previous byte of position p, key_of[p + 1] = its own byte
    if (SEG) {
        for (uint32_t i = tid; i < n; i += BK_SORT_THREADS) prev_of[i] = key_of[i];
        __syncthreads();
        bk_seg_walk(b.seg_begin, b.segs, s, len, piece == 0u ? ~0u : base + n, piece == 0u, b.bt_first, b.n_btypes, b.status, wsum,
                    [&](uint32_t q, uint32_t, uint64_t l8) { if (q - base < n) prev_of[q - base] = (uint8_t)(l8 >> 56); });
        __syncthreads();
    }
    // ONE ranking pass: wave w owns positions [2048 w, 2048 w + 2048) of the piece and visits them in order, 64 at a time.  The lanes
    // that hold the same key find each other through the wave's 256 lane masks in LDS (in `staging`, which is free until placement):
    // every lane clears its key's mask, ORs its own bit in and reads the mask back -- three LDS operations in program order, against the
    // eight ballots with a 64-bit select per lane and bit that this walk used to cost.  The mask gives the position's rank among the 64
    // positions' equal keys and the size of that key group; hist[w][key] holds the number of the wave's earlier positions with the key
    // (the last lane of each key group adds the group's size: those lanes hold distinct keys, and a wave's LDS accesses stay in program
    // order), so hist-before + rank is the position's rank among ALL of the wave's positions of its key: at most 2047, kept in
    // registers, two per dword.
    unsigned long long* mask_of = staging64 + w * 256u;     // relaxed atomics below: lanes meet in these words, nothing may be forwarded
    const unsigned long long my_bit = 1ull << lane;
    uint32_t kept[16];
#pragma unroll
    for (uint32_t bt = 0; bt < 32u; ++bt) {
        uint32_t r = 0;
        const uint32_t p = w * 2048u + bt * 64u + lane;
        if (p < n) {
            const uint32_t key = SEG ? prev_of[p] : key_of[p];
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
            const uint32_t key = SEG ? prev_of[p] : key_of[p], byte = key_of[p + 1u];
            const uint32_t slot = hist[w][key] + ((kept[bt >> 1] >> (16u * (bt & 1u))) & 0xffffu);
            staging[slot] = (uint8_t)byte;
            inv[p] = (uint16_t)slot;
        }
    }
    __syncthreads();
    uint8_t* sorted = b.sorted + (size_t)s * pl + base;
    for (uint32_t i = tid * 16u; i < n; i += BK_SORT_THREADS * 16u) {
        if (i + 16u <= n) *(u32x4*)(sorted + i) = *(const u32x4*)(staging + i);
        else for (uint32_t k = i; k < n; ++k) sorted[k] = staging[k];
    }
}

// (instantiated here, the SEG instance where launch_bucket_model names it -- behind every other kernel of the file: the kernels of
// the default path keep their places in the code object)
template __global__ void bucket_sort_kernel<false>(const BucketBatch b);

// ---------------------------------------------------------------------------------------------
// 2. task lists by bucket size class, so that the long chains start first
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void bucket_tasks_kernel(const BucketBatch b) {
    __shared__ uint32_t cnt[BK_CLASSES], basev[BK_CLASSES];
    const uint32_t t = blockIdx.x * 1024u + threadIdx.x;      // stream * 256 + prev
    const uint32_t cap = b.n_streams * 256u;
    if (threadIdx.x < BK_CLASSES) cnt[threadIdx.x] = 0u;
    __syncthreads();
    uint32_t tot = 0;
    if (t < cap) {
        const u32x4* d = (const u32x4*)(b.desc + (size_t)t * 8u);
        const u32x4 d0 = d[0], d1 = d[1];
        tot = (d0.x >> 16) + (d0.y >> 16) + (d0.z >> 16) + (d0.w >> 16) + (d1.x >> 16) + (d1.y >> 16) + (d1.z >> 16) + (d1.w >> 16);
    }
    const int cls = bk_class_of(tot);
    // slot inside the block: one LDS atomic per wave and class, then one global atomic per block and class
    uint32_t local = 0;
    for (int c = 0; c < (int)BK_CLASSES; ++c) {
        const unsigned long long m = __ballot(cls == c);
        if (m == 0ull) continue;
        const int leader = __ffsll((long long)m) - 1;
        uint32_t wbase = 0;
        if ((int)(threadIdx.x & 63u) == leader) wbase = atomicAdd(&cnt[c], (uint32_t)__popcll(m));
        wbase = (uint32_t)__builtin_amdgcn_readlane((int)wbase, leader);
        if (cls == c) local = wbase + lanes_below(m);
    }
    __syncthreads();
    if (threadIdx.x < BK_CLASSES) basev[threadIdx.x] = cnt[threadIdx.x] ? atomicAdd(&b.counters[threadIdx.x], cnt[threadIdx.x]) : 0u;
    __syncthreads();
    if (cls >= 0) b.tasks[(size_t)cls * cap + basev[cls] + local] = t;
}

// ---------------------------------------------------------------------------------------------
// 3. chains.  This kernel holds the chain loop as its OWN text: the same loop, statement for statement, as bk_chain_loop
//    (lit_bucket_dev.h), which both two-model chain kernels run and where the reasons for its shape are written down; change the
//    two together.  On bk_chain_loop this kernel compiles to other instructions and its pass measured 0.35-0.75 ms slower per
//    65 536 streams (profiles/r09_bench_ab.txt).  The group store and the row reset are shared: they leave its instructions as they were.
// ---------------------------------------------------------------------------------------------
constexpr uint32_t BK_LANE_DWORDS = 148;     // 17 rows x 8 dwords + 8 descriptors, padded: 16-byte aligned and the
                                             // 64 lanes' b128 accesses at equal offsets cover all 32 banks
constexpr uint32_t BK_DESC_DW = 136;
constexpr uint32_t BK_TAB_DW = 64 * BK_LANE_DWORDS;
__global__ __launch_bounds__(64) void bucket_chain_kernel(const BucketBatch b) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds32[];
    const uint32_t lane = threadIdx.x;
    uint32_t* my = lds32 + lane * BK_LANE_DWORDS;
    uint32_t* mydesc = my + BK_DESC_DW;
    uint32_t* tab = lds32 + BK_TAB_DW;
    const uint32_t inc = (uint32_t)b.inc; const int lim = b.lim;
    for (uint32_t i = lane; i < 128u; i += 64u) {
        tab[i] = bk_tab_entry(i, inc);
    }
    __syncthreads();
    const size_t pl = b.slot;
    const uint32_t cap = b.n_streams * 256u;
    BkTaskLists lists; lists.load(b.counters);
    const uint32_t total = lists.total();

    // per-lane chain state
    bool has_task = false, exhausted = false;
    uint32_t run_i = 0, nruns = 0, left = 0, idx = 0;
    u32x2* cur_sfs = b.sfs; const uint8_t* cur_sorted = b.sorted;   // the current bucket's stream slot
    uint32_t nt_stage = 0, nt_tid = 0;
    u32x4 nd0 = {0u, 0u, 0u, 0u}, nd1 = {0u, 0u, 0u, 0u};
    // wave-uniform task window
    uint32_t win_cur = 0, win_end = 0, nxt_val = 0, nxt_w = 0;
    const uint32_t long_end = lists.ends[3];     // tasks of at least 2048 positions come first
    bool nxt_pending = false, drained = false;
    u32x2 e_next = {0u, 0u}; uint32_t m_next = 0;           // meta: base | first << 16 | cnt << 20 | BK_VALID
    u32x2 pv0 = {0u, 0u}, pv1 = pv0, pv2 = pv0, pv3 = pv0, pv4 = pv0, pv5 = pv0, pv6 = pv0, pv7 = pv0;
    uint32_t m_prev = 0; u32x2* sfs_prev = b.sfs;

#define BK_OPAQUE(X) asm volatile("" : "+v"(X))
#define BK_BYTE(K, WORD, PV)                                                                            \
    if (((K - first) & 15u) < cnt) {                                                                    \
        const uint32_t byte_ = (WORD >> (8u * (K & 3u))) & 0xffu;                                       \
        const uint32_t hi = byte_ >> 4, lo = byte_ & 15u;                                               \
        uint32_t* rowl = my + 8u * (1u + hi);                                                           \
        BkRow H = bk_read(my, tab, hi), L = bk_read(rowl, tab, lo);                                     \
        const u32x2 v = {bk_pack(H, hi), bk_pack(L, lo)};                                               \
        bk_add(H); bk_add(L);                                                                           \
        bk_renorm_at(H, lim); bk_renorm_at(L, lim);                                                     \
        *(u32x4*)my = H.w0; *(u32x4*)(my + 4) = H.w1; *(u32x4*)rowl = L.w0; *(u32x4*)(rowl + 4) = L.w1; \
        PV = v;                                                                                         \
    }

    for (;;) {
        u32x2 e = e_next; const uint32_t m = m_next;
        // 1. the previous group's pairs leave (their registers are free again below)
#if DIVANS_BK_CHAIN_NO_STORES
        asm volatile("" : : "v"(pv0), "v"(pv1), "v"(pv2), "v"(pv3), "v"(pv4), "v"(pv5), "v"(pv6), "v"(pv7), "v"(sfs_prev));
        if (false) {
#else
        if (m_prev & BK_VALID) {
#endif
            bk_store_group(sfs_prev, m_prev, pv0, pv1, pv2, pv3, pv4, pv5, pv6, pv7);
        }
        // 2. the next group of the run is requested, the next run taken
        {
            const bool adv = has_task && left == 0u, more = run_i < nruns;
            const uint32_t d = mydesc[run_i & 7u];
            if (adv && more) { left = d >> 16; idx = d & 0xffffu; ++run_i; }
            if (adv && !more) has_task = false;
        }
        {
            const bool fetch_ = has_task && left != 0u;
            const uint32_t base = idx & ~7u, first_ = idx & 7u;
            const uint32_t cnt_ = left < 8u - first_ ? left : 8u - first_;
            const uint8_t* lp = fetch_ ? cur_sorted + base : b.sorted;
            e_next = *(const u32x2*)lp;
            m_next = fetch_ ? (base | (first_ << 16) | (cnt_ << 20) | BK_VALID) : 0u;
            idx += fetch_ ? cnt_ : 0u; left -= fetch_ ? cnt_ : 0u;
        }
        // 3. this iteration's group
        BK_OPAQUE(e);      /* keeps the compiler from touching the bytes (and waiting for them) before this point */
        m_prev = m; sfs_prev = cur_sfs;
        if (m & BK_VALID) {
            const uint32_t first = (m >> 16) & 15u, cnt = (m >> 20) & 15u;
            BK_BYTE(0u, e.x, pv0) BK_BYTE(1u, e.x, pv1) BK_BYTE(2u, e.x, pv2) BK_BYTE(3u, e.x, pv3)
            BK_BYTE(4u, e.y, pv4) BK_BYTE(5u, e.y, pv5) BK_BYTE(6u, e.y, pv6) BK_BYTE(7u, e.y, pv7)
        }
        // 4. a finished lane takes its prefetched task
        if (!has_task && !(m_next & BK_VALID) && nt_stage == 3u) {
            BK_OPAQUE(nd0); BK_OPAQUE(nd1);
            uint32_t n = 0;
            const uint32_t dsc[8] = {nd0.x, nd0.y, nd0.z, nd0.w, nd1.x, nd1.y, nd1.z, nd1.w};
#pragma unroll
            for (uint32_t j = 0; j < 8u; ++j) if (dsc[j] >> 16) { mydesc[n] = dsc[j] + j * BK_PIECE; ++n; }   // first slot + piece base < 65536
            nruns = n; run_i = 0u;
            bk_rows_reset(my, 17u);
            cur_sfs = b.sfs + (size_t)(nt_tid >> 8) * pl; cur_sorted = b.sorted + (size_t)(nt_tid >> 8) * pl;
            left = 0u; has_task = true; nt_stage = 0u;
        }
        // task prefetch pipeline, one stage per iteration so that no load is waited for in the iteration that issued it
        const bool want = nt_stage == 0u && !exhausted;
        if (nt_stage == 2u) nt_stage = 3u;
        else if (nt_stage == 1u) {
            BK_OPAQUE(nt_tid);
            const u32x4* dp = (const u32x4*)(b.desc + (size_t)nt_tid * 8u);
            nd0 = dp[0]; nd1 = dp[1];
            nt_stage = 2u;
        }
        const unsigned long long wm = __ballot(want);
        if (wm) {
            if (win_cur == win_end && nxt_pending) {
                BK_OPAQUE(nxt_val);
                const uint32_t basev = (uint32_t)__builtin_amdgcn_readfirstlane((int)nxt_val);
                nxt_pending = false;
                if (basev >= total) { drained = true; win_cur = win_end = total; }
                else { win_cur = basev; win_end = basev + nxt_w < total ? basev + nxt_w : total; }
            }
            const uint32_t avail = win_end - win_cur, asked = (uint32_t)__popcll(wm);
            const uint32_t rank = lanes_below(wm);
            if (want) {
                if (rank < avail) {
                    const uint32_t t = win_cur + rank;
                    nt_tid = *lists.at(b.tasks, cap, t);
                    nt_stage = 1u;
                } else if (drained) exhausted = true;
            }
            win_cur += asked < avail ? asked : avail;
        }
        // long buckets are handed out 64 at a time: a wave that reserved 256 of them would run four per lane back to back
        const uint32_t want_w = win_end < long_end ? 64u : BK_WINDOW;
        if (!nxt_pending && !drained && win_end - win_cur < want_w / 2u) {
            nxt_w = want_w;
            if (lane == 0u) nxt_val = atomicAdd(&b.counters[BK_CLAIM], want_w);
            nxt_pending = true;
        }
        const bool done = !has_task && !(m_next & BK_VALID) && !(m_prev & BK_VALID) && nt_stage == 0u && exhausted;
        if (__ballot(!done) == 0ull) break;
    }
#undef BK_BYTE
#undef BK_OPAQUE
}

// ---------------------------------------------------------------------------------------------
// 4. back to position order: sf[stream][pos] = sfs[stream][piece][inv[pos]]
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void bucket_unsort_kernel(const BucketBatch b) {
    __shared__ u32x2 buf[BK_PIECE];
    const uint32_t s = blockIdx.x / b.pieces, piece = blockIdx.x % b.pieces;
    const uint32_t len = b.in_sizes ? b.in_sizes[s] : b.stream_len;
    const uint32_t base = piece * BK_PIECE;
    if (base >= len) return;
    const uint32_t n = len - base < BK_PIECE ? len - base : BK_PIECE;
    const size_t pl = b.slot;
    const u32x2* src = b.sfs + (size_t)s * pl + base;
    for (uint32_t i = threadIdx.x; i < n; i += 1024u) buf[i] = __builtin_nontemporal_load(src + i);
    __syncthreads();
    const uint16_t* inv = b.inv + (size_t)s * pl + base;
    u32x2* dst = (u32x2*)(b.sf + (size_t)s * b.sf_stride) + base;
    for (uint32_t i = threadIdx.x; i < n; i += 1024u) dst[i] = buf[inv[i]];
}

// the same for a plane of 4-byte elements (the two-model pass's maxes): sfs / sf are read as uint32_t arrays, `slot` / sf_stride apart
__global__ __launch_bounds__(1024) void bucket_unsort32_kernel(const BucketBatch b) {
    __shared__ uint32_t buf[BK_PIECE];
    const uint32_t s = blockIdx.x / b.pieces, piece = blockIdx.x % b.pieces;
    const uint32_t len = b.in_sizes ? b.in_sizes[s] : b.stream_len;
    const uint32_t base = piece * BK_PIECE;
    if (base >= len) return;
    const uint32_t n = len - base < BK_PIECE ? len - base : BK_PIECE;
    const size_t pl = b.slot;
    const uint32_t* src = (const uint32_t*)b.sfs + (size_t)s * pl + base;
    const uint32_t n2 = (n + 1u) & ~1u;                    // pieces start on even elements and the slot is even: whole pairs
    for (uint32_t i = 2u * threadIdx.x; i < n2; i += 2048u) *(u32x2*)(buf + i) = __builtin_nontemporal_load((const u32x2*)(src + i));
    __syncthreads();
    const uint16_t* inv = b.inv + (size_t)s * pl + base;
    uint32_t* dst = b.sf + (size_t)s * b.sf_stride + base;
    for (uint32_t i = 2u * threadIdx.x; i < n2; i += 2048u) {
        const uint32_t iv = *(const uint32_t*)(inv + i);
        const u32x2 v = {buf[iv & 0xffffu], i + 1u < n ? buf[iv >> 16] : 0u};
        *(u32x2*)(dst + i) = v;
    }
}

// ---------------------------------------------------------------------------------------------
// 1'. the sort for a stride distance D = dist in {2, 3, 4, 8} (mixing values 5, 6, 7 and 8 and above under a constant context: high
//     row [ctx][b_D], low row [b_D][hi] with b_D the byte D places back, literal.rs:184-208): the key of position p is in[p - D], and 0
//     for p < D (a fresh stream's last_8_literals is zero; nothing in front of the stream is read).  A piece needs the D bytes in
//     front of its base: piece_in[16 - D .. 16).
//     SEG: position j < min(D, len) of a segment takes its key from the segment's last8 at distance D - j -- the byte lane
//     bucket_sort_kernel<true> reads distance 1 from; a segment shorter than D hands nothing on (the next one brings its own last8),
//     and a segment that starts up to D - 1 positions before the piece base still patches the keys that fall into this piece.
//     Ranking, scan and placement are bk_sort_piece (lit_bucket_dev.h); tasks, chains and unsort never look at what the key was.
// ---------------------------------------------------------------------------------------------
template <bool SEG>
__global__ __launch_bounds__(BK_SORT_THREADS) void bucket_sort_stride_kernel(const BucketBatch b, const uint32_t dist) {
    __shared__ __attribute__((aligned(16))) unsigned long long staging64[BK_PIECE / 8u];
    __shared__ __attribute__((aligned(16))) uint8_t piece_in[16 + BK_PIECE];
    __shared__ uint32_t hist[4][256];
    __shared__ uint32_t wsum[4];
    __shared__ uint8_t key_lds[SEG ? BK_PIECE : 1u];     // SEG: the key of every position
    const uint32_t s = blockIdx.x / b.pieces, piece = blockIdx.x % b.pieces;
    const uint32_t tid = threadIdx.x;
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
    for (uint32_t i = tid; i < 1024u; i += BK_SORT_THREADS) (&hist[0][0])[i] = 0u;
    bk_load_piece(piece_in, in + base, n);
    if (tid < dist) piece_in[16u - dist + tid] = base ? in[base - dist + tid] : 0u;     // base >= 8192 > dist, or the stream's start
    __syncthreads();
    const uint8_t* key_of = piece_in + 16u - dist;      // key_of[p] = the byte dist places before position p
    if (SEG) {
        for (uint32_t i = tid; i < n; i += BK_SORT_THREADS) key_lds[i] = key_of[i];
        __syncthreads();
        bk_seg_walk(b.seg_begin, b.segs, s, len, piece == 0u ? ~0u : base + n, piece == 0u, b.bt_first, b.n_btypes, b.status, wsum,
                    [&](uint32_t q, uint32_t l, uint64_t l8) {
                        const uint32_t own = l < dist ? l : dist;
                        for (uint32_t j = 0; j < own; ++j)      // q + j - base wraps above n for a position in front of the piece
                            if (q + j - base < n) key_lds[q + j - base] = (uint8_t)(l8 >> (64u - 8u * (dist - j)));
                    });
        __syncthreads();
    }
    bk_sort_piece(b, s, base, n, desc, SEG ? key_lds : key_of, piece_in + 16, staging64, hist, wsum);
}

uint32_t bucket_chain_lds_bytes() { return (64u * BK_LANE_DWORDS + 128u) * 4u; }

// steps 2 and 4 on their own, for the two-model pass (lit_bucket_mix.hip) that brings its own sort and chain kernels
void launch_bucket_tasks(const BucketBatch& b, hipStream_t st) {
    hipLaunchKernelGGL(bucket_tasks_kernel, dim3((b.n_streams + 3u) / 4u), dim3(1024), 0, st, b);
}
// step 3 on its own, for the context-keyed pass (lit_bucket_ctx.hip): its buckets have this kernel's 17 rows
void launch_bucket_chain(const BucketBatch& b, uint32_t chain_blocks, hipStream_t st) {
    hipLaunchKernelGGL(bucket_chain_kernel, dim3(chain_blocks), dim3(64), bucket_chain_lds_bytes(), st, b);
}
void launch_bucket_unsort(const BucketBatch& b, hipStream_t st) {
    hipLaunchKernelGGL(bucket_unsort_kernel, dim3(b.n_streams * b.pieces), dim3(1024), 0, st, b);
}

void launch_bucket_unsort32(const BucketBatch& b, hipStream_t st) {
    hipLaunchKernelGGL(bucket_unsort32_kernel, dim3(b.n_streams * b.pieces), dim3(1024), 0, st, b);
}

hipError_t launch_bucket_model(const BucketBatch& b, uint32_t chain_blocks, hipStream_t st) {
    hipError_t e = hipMemsetAsync(b.counters, 0, 64, st);
    if (e != hipSuccess) return e;
    if (b.pieces < 8u) {
        e = hipMemsetAsync(b.desc, 0, (size_t)b.n_streams * 256u * 8u * sizeof(uint32_t), st);
        if (e != hipSuccess) return e;
    }
    if (b.segs) hipLaunchKernelGGL(bucket_sort_kernel<true>, dim3(b.n_streams * b.pieces), dim3(BK_SORT_THREADS), 0, st, b);
    else hipLaunchKernelGGL(bucket_sort_kernel<false>, dim3(b.n_streams * b.pieces), dim3(BK_SORT_THREADS), 0, st, b);
    hipLaunchKernelGGL(bucket_tasks_kernel, dim3((b.n_streams + 3u) / 4u), dim3(1024), 0, st, b);
#if DIVANS_BK_CHAIN_NO_STORES   // every pair reads (start 1, freq 2048): the rANS pass stays inside its slots on the pairs nobody wrote
    e = hipMemsetD32Async((hipDeviceptr_t)b.sfs, (int)(1u | (2048u << 16)), (size_t)b.n_streams * b.slot * 2u, st);
    if (e != hipSuccess) return e;
#endif
    hipLaunchKernelGGL(bucket_chain_kernel, dim3(chain_blocks), dim3(64), bucket_chain_lds_bytes(), st, b);
    hipLaunchKernelGGL(bucket_unsort_kernel, dim3(b.n_streams * b.pieces), dim3(1024), 0, st, b);
    return hipGetLastError();
}

// launch_bucket_model with the stride sort in place of bucket_sort_kernel (its instances behind every other kernel of the file)
hipError_t launch_bucket_stride_model(const BucketBatch& b, uint32_t dist, uint32_t chain_blocks, hipStream_t st) {
    if (!(dist == 2u || dist == 3u || dist == 4u || dist == 8u)) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(b.counters, 0, 64, st);
    if (e != hipSuccess) return e;
    if (b.pieces < 8u) {
        e = hipMemsetAsync(b.desc, 0, (size_t)b.n_streams * 256u * 8u * sizeof(uint32_t), st);
        if (e != hipSuccess) return e;
    }
    if (b.segs) hipLaunchKernelGGL(bucket_sort_stride_kernel<true>, dim3(b.n_streams * b.pieces), dim3(BK_SORT_THREADS), 0, st, b, dist);
    else hipLaunchKernelGGL(bucket_sort_stride_kernel<false>, dim3(b.n_streams * b.pieces), dim3(BK_SORT_THREADS), 0, st, b, dist);
    launch_bucket_tasks(b, st);
    launch_bucket_chain(b, chain_blocks, st);
    launch_bucket_unsort(b, st);
    return hipGetLastError();
}

}  // namespace divans_hip
