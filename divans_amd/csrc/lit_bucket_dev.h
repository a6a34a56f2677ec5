// lit_bucket_dev.h -- device code shared by the bucketed encoder passes (lit_bucket.hip, lit_bucket_mix.hip): the sort kernels'
// piece load and segment walk, the arithmetic of one nibble against a packed row, the chain kernels' group
// store and row reset, and bk_chain_loop -- the loop of a chain kernel (task window, task prefetch, run cursor, delayed stores) that
// both mix_chain_kernel<MODEL> instances fill with their per-position work; bucket_chain_kernel (lit_bucket.hip) holds the same loop
// as its own text, see there.
#ifndef DIVANS_LIT_BUCKET_DEV_H_
#define DIVANS_LIT_BUCKET_DEV_H_
#include <type_traits>
#include "lit_device.h"

namespace divans_hip {

constexpr uint32_t BK_PIECE = 8192;          // positions sorted together
constexpr uint32_t BK_SORT_THREADS = 256;
constexpr uint32_t BK_VALID = 1u << 31;
constexpr uint32_t BK_WINDOW = 256;          // tasks a wave reserves per atomic
constexpr uint32_t BK_CLASSES = 6;           // task lists by bucket size, longest first (a bucket is a serial chain: the long ones must start early)
constexpr uint32_t BK_CLAIM = 8;             // counters[0..5] = tasks per class, counters[BK_CLAIM] = next unclaimed task

__device__ __forceinline__ int bk_class_of(uint32_t tot) {
    return tot == 0u ? -1 : (tot >= 16384u ? 0 : (tot >= 8192u ? 1 : (tot >= 4096u ? 2 : (tot >= 2048u ? 3 : (tot >= 64u ? 4 : 5)))));
}
// the t-th task overall: class lists are [BK_CLASSES][cap], `ends` their cumulative sizes
struct BkTaskLists {
    uint32_t ends[BK_CLASSES];
    __device__ __forceinline__ void load(const uint32_t* counters) {
        uint32_t acc = 0;
#pragma unroll
        for (uint32_t c = 0; c < BK_CLASSES; ++c) { acc += counters[c]; ends[c] = acc; }
    }
    __device__ __forceinline__ uint32_t total() const { return ends[BK_CLASSES - 1u]; }
    __device__ __forceinline__ const uint32_t* at(const uint32_t* tasks, uint32_t cap, uint32_t t) const {
        uint32_t cls = 0, base = 0;
#pragma unroll
        for (uint32_t c = 0; c + 1u < BK_CLASSES; ++c) if (t >= ends[c]) { cls = c + 1u; base = ends[c]; }
        return tasks + (size_t)cls * cap + (t - base);
    }
};

__device__ __forceinline__ uint32_t lanes_below(unsigned long long m) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// the piece's n bytes once into LDS at piece_in + 16 (the bytes before the piece go in front of them), 16 bytes per lane where
// alignment allows
__device__ __forceinline__ void bk_load_piece(uint8_t* piece_in, const uint8_t* src, uint32_t n) {
    const uint32_t tid = threadIdx.x;
    if ((((uintptr_t)src) & 15u) == 0u) {
        for (uint32_t i = tid * 16u; i < n; i += BK_SORT_THREADS * 16u) {
            if (i + 16u <= n) *(u32x4*)(piece_in + 16u + i) = *(const u32x4*)(src + i);
            else for (uint32_t k = i; k < n; ++k) piece_in[16u + k] = src[k];
        }
    } else {
        for (uint32_t i = tid; i < n; i += BK_SORT_THREADS) piece_in[16u + i] = src[i];
    }
}

// The SEG = true sort kernels: the whole workgroup (BK_SORT_THREADS lanes) walks the segment list of ITS stream, 256 segments per
// step with a block-wide running sum of `len`, and calls patch(q, len, last8) -- by the lane that holds the segment -- for every
// NON-EMPTY segment that starts at an offset q below the stream's length: such a segment installs its last8 as the history of
// position q (SegCursor::advance, lit_device.h; empty segments install nothing that lasts).  The walk ends after the step in which
// the running sum passes `until` (no later segment starts below it).  With `check` (one workgroup per stream: until = ~0u) it walks
// the whole list and raises LIT_STATUS_BAD_SEGMENT where the lengths do not add up to `len` or a segment names a block type outside
// [bt_first, bt_first + n_btypes).  A length is clamped to 65 537 (> any stream of the bucketed passes: the verdict is the same) and
// the walk stops once the sum has passed the stream's length, so the sum stays far inside 32 bits however long the list is.
// `wsum` = four words of LDS; every lane of the workgroup must call this (it synchronises).
// A patch that takes a fourth argument also receives the segment's block type as the list names it (ctx_sort_kernel, lit_bucket_ctx.hip).
template <class Patch>
__device__ __forceinline__ void bk_seg_walk(const uint32_t* seg_begin, const LitSegment* segs, uint32_t s, uint32_t len, uint32_t until, bool check,
                                            uint32_t bt_first, uint32_t n_btypes, uint32_t* status, uint32_t* wsum, Patch&& patch) {
    const uint32_t tid = threadIdx.x, w = tid >> 6, lane = tid & 63u;
    const uint32_t first = seg_begin[s], end = seg_begin[s + 1u];
    uint32_t run = 0u;
    bool bad = false;
    for (uint32_t i0 = first; i0 < end; i0 += BK_SORT_THREADS) {       // workgroup-uniform
        const uint32_t i = i0 + tid;
        u32x4 sg = {0u, 0u, 0u, 0u};
        if (i < end) {
            sg = *(const u32x4*)(segs + i);
            if (sg.y - bt_first >= n_btypes) bad = true;
        }
        const uint32_t l = sg.x < 65537u ? sg.x : 65537u;
        uint32_t incl = l;
        for (uint32_t d = 1; d < 64u; d <<= 1) {
            const uint32_t v = (uint32_t)__shfl_up((int)incl, d, 64);
            if (lane >= d) incl += v;
        }
        if (lane == 63u) wsum[w] = incl;
        __syncthreads();
        const uint32_t s0 = wsum[0], s1 = wsum[1], s2 = wsum[2], s3 = wsum[3];
        const uint32_t q = run + (w > 0u ? s0 : 0u) + (w > 1u ? s1 : 0u) + (w > 2u ? s2 : 0u) + incl - l;
        if (l != 0u && q < len) {
            if constexpr (std::is_invocable_v<Patch&, uint32_t, uint32_t, uint64_t, uint32_t>) patch(q, l, ((uint64_t)sg.w << 32) | sg.z, sg.y);
            else patch(q, l, ((uint64_t)sg.w << 32) | sg.z);
        }
        run += s0 + s1 + s2 + s3;
        __syncthreads();
        if (run > len || run >= until) break;
    }
    if (check) {
        if (bad || (run != len && tid == 0u)) atomicOr(status, LIT_STATUS_BAD_SEGMENT);
    }
}

// What a sort kernel of lit_bucket.hip does once the keys of a piece are known: keys[p] (LDS) = the bucket key of position p of
// the piece, bytes[p] (LDS) = its byte, n positions.  bucket_sort_stride_kernel runs it; bucket_sort_kernel holds the same
// statements as its own text (on this function it compiles to other instructions, and the kernels of the default path keep theirs):
// change the two together.  Leaves sorted / inv of the piece and *desc = first slot | count << 16 of key
// threadIdx.x.  staging64 (BK_PIECE bytes), hist ([4][256], zeroed by the caller), wsum (4 words): LDS of the workgroup of
// BK_SORT_THREADS lanes, all of which call this behind a barrier that has made keys, bytes and hist visible.
__device__ __forceinline__ void bk_sort_piece(const BucketBatch& b, uint32_t s, uint32_t base, uint32_t n, uint32_t* desc, const uint8_t* keys,
                                              const uint8_t* bytes, unsigned long long* staging64, uint32_t (*hist)[256], uint32_t* wsum) {
    uint8_t* staging = (uint8_t*)staging64;
    const uint32_t tid = threadIdx.x, w = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6)), lane = tid & 63;
    const size_t pl = b.slot;
    // ONE ranking pass over the wave's 256 lane masks in LDS, as explained in bucket_sort_kernel
    unsigned long long* mask_of = staging64 + w * 256u;     // relaxed atomics below: lanes meet in these words, nothing may be forwarded
    const unsigned long long my_bit = 1ull << lane;
    uint32_t kept[16];
#pragma unroll
    for (uint32_t bt = 0; bt < 32u; ++bt) {
        uint32_t r = 0;
        const uint32_t p = w * 2048u + bt * 64u + lane;
        if (p < n) {
            const uint32_t key = keys[p];
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
            const uint32_t key = keys[p], byte = bytes[p];
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

// One nibble against a row of 8 dwords (16 x u16) in LDS, split into phases so that the two nibbles of a byte
// (different rows) can be in flight together: read, pack (start | freq << 16), blend, write.
struct BkRow { u32x4 w0, w1, a0, a1; int chi, cprev; };

__device__ __forceinline__ BkRow bk_read(const uint32_t* row, const uint32_t* tab, uint32_t sym) {
    BkRow r;
    r.w0 = *(const u32x4*)row; r.w1 = *(const u32x4*)(row + 4);
    const uint16_t* r16 = (const uint16_t*)row;
    r.chi = r16[sym];
    r.cprev = r16[sym ? sym - 1u : 0u];
    r.a0 = *(const u32x4*)(tab + sym * 8u); r.a1 = *(const u32x4*)(tab + sym * 8u + 4u);
    return r;
}
__device__ __forceinline__ uint32_t bk_pack(const BkRow& r, uint32_t sym) {     // probability/interface.rs:97-108
    const int mx = (int)(r.w1.w >> 16);
    const int clo = sym ? r.cprev : 0;
    const float rcp = biased_rcp15(mx);
    const uint32_t dhi = scaled_div(r.chi, mx, rcp), dlo = scaled_div(clo, mx, rcp);
    return (dlo + 1u) | ((dhi - dlo - 1u) << 16);
}
__device__ __forceinline__ void bk_renorm(BkRow& r) {                           // frequentist_cdf.rs:79-84, both halves at once
    const u32x4 b0 = {1u | (2u << 16), 3u | (4u << 16), 5u | (6u << 16), 7u | (8u << 16)};
    const u32x4 b1 = {9u | (10u << 16), 11u | (12u << 16), 13u | (14u << 16), 15u | (16u << 16)};
    const u32x4 t0 = r.w0 + b0, t1 = r.w1 + b1;
    r.w0 = t0 - ((t0 >> 2) & 0x3fff3fffu);
    r.w1 = t1 - ((t1 >> 2) & 0x3fff3fffu);
}

// frequentist_cdf.rs:74-85 on the packed row: the add of the symbol's increment row (bk_read fetched it from the table
// bk_tab_entry fills), then the renormalisation once the NEW total has reached the speed's limit
__device__ __forceinline__ uint32_t bk_tab_entry(uint32_t i, uint32_t inc) {    // dword k = i & 7 of symbol i >> 3: entries 2k and 2k + 1 take `inc` from the symbol up
    const uint32_t sym = i >> 3, k = i & 7u;
    return (2u * k >= sym ? inc : 0u) | (2u * k + 1u >= sym ? inc << 16 : 0u);
}
__device__ __forceinline__ void bk_add(BkRow& r) { r.w0 += r.a0; r.w1 += r.a1; }              // frequentist_cdf.rs:75-78
__device__ __forceinline__ void bk_renorm_at(BkRow& r, int lim) { if ((int)(r.w1.w >> 16) >= lim) bk_renorm(r); }

__device__ __forceinline__ void bk_store_quad(u32x4* p, u32x4 v) {     // 8-byte aligned is enough for a global store
    asm volatile("global_store_dwordx4 %0, %1, off" : : "v"(p), "v"(v) : "memory");
}
__device__ __forceinline__ void bk_store_pair(u32x2* p, u32x2 v) {
    asm volatile("global_store_dwordx2 %0, %1, off" : : "v"(p), "v"(v) : "memory");
}
__device__ __forceinline__ void bk_store_word(uint32_t* p, uint32_t v) {
    asm volatile("global_store_dword %0, %1, off" : : "v"(p), "v"(v) : "memory");
}


// a fresh CDF row (entry i = 4 (i + 1)) into each of the `nrows` rows at `rows`
__device__ __forceinline__ void bk_rows_reset(uint32_t* rows, uint32_t nrows) {
    const u32x4 def0 = {4u | (8u << 16), 12u | (16u << 16), 20u | (24u << 16), 28u | (32u << 16)};
    const u32x4 def1 = {36u | (40u << 16), 44u | (48u << 16), 52u | (56u << 16), 60u | (64u << 16)};
    for (uint32_t r = 0; r < nrows; ++r) { *(u32x4*)(rows + 8u * r) = def0; *(u32x4*)(rows + 8u * r + 4u) = def1; }
}

// The eight values r0 .. r7 of the group `m` describes (base | first << 16 | cnt << 20) leave for plane[base ..]: a full group as
// 16-byte stores, otherwise the positions the run owns one by one.  T = u32x2 (pairs) or uint32_t (words).
__device__ __forceinline__ void bk_store_one(u32x2* p, u32x2 v) { bk_store_pair(p, v); }
__device__ __forceinline__ void bk_store_one(uint32_t* p, uint32_t v) { bk_store_word(p, v); }
__device__ __forceinline__ void bk_store_full(u32x2* dst, u32x2 r0, u32x2 r1, u32x2 r2, u32x2 r3, u32x2 r4, u32x2 r5, u32x2 r6, u32x2 r7) {
    const u32x4 q0 = {r0.x, r0.y, r1.x, r1.y}, q1 = {r2.x, r2.y, r3.x, r3.y};
    const u32x4 q2 = {r4.x, r4.y, r5.x, r5.y}, q3 = {r6.x, r6.y, r7.x, r7.y};
    bk_store_quad((u32x4*)dst, q0); bk_store_quad((u32x4*)(dst + 2), q1);
    bk_store_quad((u32x4*)(dst + 4), q2); bk_store_quad((u32x4*)(dst + 6), q3);
}
__device__ __forceinline__ void bk_store_full(uint32_t* dst, uint32_t r0, uint32_t r1, uint32_t r2, uint32_t r3, uint32_t r4, uint32_t r5, uint32_t r6, uint32_t r7) {
    const u32x4 q0 = {r0, r1, r2, r3}, q1 = {r4, r5, r6, r7};
    bk_store_quad((u32x4*)dst, q0); bk_store_quad((u32x4*)(dst + 4), q1);
}
template <class T>
__device__ __forceinline__ void bk_store_group(T* plane, uint32_t m, T r0, T r1, T r2, T r3, T r4, T r5, T r6, T r7) {
    T* dst = plane + (m & 0xffffu);
    const uint32_t pf = (m >> 16) & 15u, pc = (m >> 20) & 15u;
    if (pc == 8u) {
        bk_store_full(dst, r0, r1, r2, r3, r4, r5, r6, r7);
    } else {
        if (((0u - pf) & 15u) < pc) bk_store_one(dst + 0, r0);
        if (((1u - pf) & 15u) < pc) bk_store_one(dst + 1, r1);
        if (((2u - pf) & 15u) < pc) bk_store_one(dst + 2, r2);
        if (((3u - pf) & 15u) < pc) bk_store_one(dst + 3, r3);
        if (((4u - pf) & 15u) < pc) bk_store_one(dst + 4, r4);
        if (((5u - pf) & 15u) < pc) bk_store_one(dst + 5, r5);
        if (((6u - pf) & 15u) < pc) bk_store_one(dst + 6, r6);
        if (((7u - pf) & 15u) < pc) bk_store_one(dst + 7, r7);
    }
}

#define BK_OPAQUE(X) asm volatile("" : "+v"(X))     // the compiler knows nothing about X before this point (undefined again below the loop)

// The loop of a chain kernel: ONE LANE per bucket walks the bucket's positions in order with the bucket's rows in LDS.  `b` is the
// kernel's batch (the fields BucketBatch and MixBucketBatch share: n_streams, slot, sorted, desc, tasks, counters); K is the kernel's
// own part, a type without state:
//   K::Group                 u32x2 / u32x4: the eight sorted payloads one load brings (b.sorted holds bytes / 16-bit payloads)
//   K::ROWS, K::Env          env.my = the lane's LDS: ROWS rows of 8 dwords, then the bucket's 8 run descriptors; the rest is K's
//   K::Slot, K::slot(b, off) where a bucket's values go: the planes of the stream whose slot starts `off` elements in
//   K::Out, K::code(...)     what the positions [first, first + cnt) of group e leave once they are blended into the rows
//   K::store(slot, m, out)   stores it where m says (bk_store_group)
//
// A bucket is up to eight runs of consecutive sorted slots, one per 8 KiB piece that holds some of its positions; the task's
// descriptors are compacted to the non-empty ones when the lane takes it (mydesc[0 .. nruns)).
// The chain is bound by the vector-memory path, not by its arithmetic (profiles/r03c_chain_role_experiment.txt), so a lane moves
// its payloads eight at a time: ONE aligned load per iteration covers the sorted slots [base, base + 8), of which the run owns
// [first, first + cnt); it is requested one iteration before it is coded.  What a group leaves goes out at the top of the NEXT
// iteration -- 16-byte stores for a full group -- through inline asm: the compiler then sees one load per iteration and waits
// for it with vmcnt(0) at a point where the only other operations in flight are stores a whole iteration old (a store is
// acknowledged out of order with loads, so no smaller count would prove the load complete).
// Every statement below is where it is on purpose (the opacity points, the step order 1-2-3-4, the prefetch one stage per iteration).
// Everything comes and goes BY VALUE, so that the compiler simplifies this loop over plain values as it would inside a kernel body.
// bucket_chain_kernel (lit_bucket.hip) holds the same loop as its own text, see there: change the two together.
template <class K, class Batch>
__device__ __forceinline__ void bk_chain_loop(const typename K::Env env, const Batch b) {
    const uint32_t lane = threadIdx.x;
    uint32_t* my = env.my;
    uint32_t* mydesc = my + 8u * K::ROWS;
    const size_t pl = b.slot;
    const uint32_t cap = b.n_streams * 256u;
    BkTaskLists lists; lists.load(b.counters);
    const uint32_t total = lists.total();

    // per-lane chain state
    bool has_task = false, exhausted = false;
    uint32_t run_i = 0, nruns = 0, left = 0, idx = 0;
    typename K::Slot cur = K::slot(b, 0u); const auto* cur_sorted = b.sorted;          // the current bucket's stream slot
    uint32_t nt_stage = 0, nt_tid = 0;
    u32x4 nd0 = {0u, 0u, 0u, 0u}, nd1 = {0u, 0u, 0u, 0u};
    // wave-uniform task window
    uint32_t win_cur = 0, win_end = 0, nxt_val = 0, nxt_w = 0;
    const uint32_t long_end = lists.ends[3];     // tasks of at least 2048 positions come first
    bool nxt_pending = false, drained = false;
    typename K::Group e_next = {}; uint32_t m_next = 0;     // meta: base | first << 16 | cnt << 20 | BK_VALID
    typename K::Out out = {};
    uint32_t m_prev = 0; typename K::Slot prev = cur;

    for (;;) {
        typename K::Group e = e_next; const uint32_t m = m_next;
        // 1. what the previous group left goes out (its registers are free again below)
        if (m_prev & BK_VALID) K::store(prev, m_prev, out);
        // 2. the next group of the run is requested (every lane issues exactly one load, from a harmless address if it has nothing
        //    to fetch), the next run of the bucket taken when this one is used up
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
            const auto* lp = fetch_ ? cur_sorted + base : b.sorted;
            e_next = *(const typename K::Group*)lp;
            m_next = fetch_ ? (base | (first_ << 16) | (cnt_ << 20) | BK_VALID) : 0u;
            idx += fetch_ ? cnt_ : 0u; left -= fetch_ ? cnt_ : 0u;
        }
        // 3. this iteration's group
        BK_OPAQUE(e);      /* keeps the compiler from touching the payloads (and waiting for them) before this point */
        m_prev = m; prev = cur;
        if (m & BK_VALID) out = K::code(env, e, (m >> 16) & 15u, (m >> 20) & 15u, out);
        // 4. a lane whose bucket is finished -- the group coded above was its last: nothing of it is still to be requested or
        //    coded, only what that group left waits for step 1 (with `prev`) -- takes its prefetched task
        if (!has_task && !(m_next & BK_VALID) && nt_stage == 3u) {
            BK_OPAQUE(nd0); BK_OPAQUE(nd1);
            uint32_t n = 0;
            const uint32_t dsc[8] = {nd0.x, nd0.y, nd0.z, nd0.w, nd1.x, nd1.y, nd1.z, nd1.w};
#pragma unroll
            for (uint32_t j = 0; j < 8u; ++j) if (dsc[j] >> 16) { mydesc[n] = dsc[j] + j * BK_PIECE; ++n; }   // first slot + piece base < 65536
            nruns = n; run_i = 0u;
            bk_rows_reset(my, K::ROWS);
            const size_t off = (size_t)(nt_tid >> 8) * pl;
            cur = K::slot(b, off); cur_sorted = b.sorted + off;
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
}
#undef BK_OPAQUE

}  // namespace divans_hip
#endif
