// fakehip_rt.cpp -- TEST HARNESS: a recording HIP runtime for the CPU (tests/c/README.md, "The launch contract").
// Defines every runtime symbol the host-only objects of divans_amd/csrc/*.hip and capi.cpp reference.  Compiled against the real HIP
// headers for their types only and never linked with libamdhip64: no kernel code runs and no GPU is touched.  Memory is address
// ranges of lazily committed anonymous mappings, so a codec with gigabytes of tables and tens of gigabytes of work arrays can be
// "allocated"; streams have a kind (null, blocking, non-blocking) and a queue whose entries carry the bytes they read and write, and two
// unordered entries of different streams on the same bytes are an `order` violation (README, "The stream model"); every launch is recorded with its argument structs and checked against the layouts
// documented in divans_amd/csrc/lit_kernels.h at once.  A violation ends the program with a message naming the kernel and the field.
#include "fakehip_rt.h"

#include <cxxabi.h>
#include <sys/mman.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <map>
#include <mutex>

#include "../../divans_amd/csrc/lit_kernels.h"

#if defined(__has_feature)
#if __has_feature(address_sanitizer)
#include <sanitizer/asan_interface.h>
#define FAKEHIP_ASAN 1
#endif
#endif

using namespace divans_hip;

namespace {

constexpr size_t kPage = 4096;
constexpr size_t kLdsPerCu = 160u * 1024u;      // MI355X
constexpr int kNumCus = 256;
constexpr size_t kGranularity = (size_t)2 << 20;
constexpr size_t kCopyLimit = (size_t)64 << 20;   // larger device-to-device copies are checked, not carried out
constexpr size_t kFillLimit = (size_t)64 << 20;   // set_fresh_fill: what is filled of a fresh block or mapped chunk, from its start (the rest stays lazily committed zero pages)
int g_fresh_fill = -1;

struct Mapping { size_t off, bytes; uint64_t handle; bool access; };
struct Range {
    uintptr_t base = 0; size_t bytes = 0; int kind = fakehip::KIND_BLOCK; int device = 0; bool alive = true;
    uint64_t born = 0, last_launch = 0;
    std::vector<Mapping> maps;      // KIND_RESERVED: what is mapped, by offset
    bool sealed = false;            // hipMemSetAccess has completed a mapping: nothing more may be mapped until all of it is gone
};
struct Phys { size_t bytes; int device; bool released; int mapped; };
typedef std::map<void*, uint64_t> Clock;        // stream -> the last entry of it that is ordered before (an edge of hipStreamWaitEvent or of the legacy null stream)
struct Event { void* stream = nullptr; uint64_t seq = 0; bool recorded = false; uint64_t id = 0; Clock clock; };
struct Failure { std::string fn; uint64_t at; hipError_t e; bool global; };
// One entry of a stream's queue (README "The stream model").  What an entry does to DEVICE memory is carried out when it is enqueued
// -- program order is one valid order of the device's work as long as the `order` rule holds, and the launch contract reads offset
// and size arrays the copies in front of a launch brought --; what the HOST can see of an entry of a non-blocking stream (the
// destination of a device-to-host copy, the end of a launch) arrives when the entry completes.
enum OpType { OP_LAUNCH, OP_COPY, OP_FILL, OP_RECORD, OP_WAIT };
struct Op {
    uint64_t id = 0; void* stream = nullptr; int type = OP_COPY; std::string what;
    uint64_t launch_seq = 0;
    std::vector<fakehip::Span> spans;
    Clock clock;
    // a device-to-host copy of a non-blocking stream: the source as it was at this place of the queue, delivered at completion
    void* dst = nullptr; size_t dpitch = 0, width = 0, height = 0; std::vector<uint8_t> staged; bool deferred = false;
    // a copy from page-locked memory reads its source when it runs: the bytes must still be those it was enqueued with
    const void* pinned_src = nullptr; std::vector<uint8_t> pinned_copy;
};
struct StreamState { int kind = fakehip::STREAM_NULL; uint64_t last = 0; Clock clock; bool alive = true; };

std::recursive_mutex g_mu;
#define LOCK std::lock_guard<std::recursive_mutex> lock_(g_mu)
std::map<uintptr_t, Range> g_ranges;           // by base; dead blocks leave (their addresses are unmapped), reserved ranges stay
std::vector<Range> g_dead;                     // freed blocks, for the ledger and for messages
std::map<uint64_t, Phys> g_phys;
uint64_t g_next_handle = 1, g_born = 0;
size_t g_capacity = (size_t)288 << 30, g_live = 0, g_reserved = 0, g_peak = 0;
int g_device = 0;
thread_local hipError_t g_last_error = hipSuccess;
std::vector<fakehip::Launch> g_launches;
std::vector<float> g_durations;                // by seq - 1
// host stub -> demangled name; filled by the module constructors of the product's objects, which may run before this file's own
std::map<const void*, std::string>& kernels() { static auto* m = new std::map<const void*, std::string>(); return *m; }
std::map<const void*, int> g_max_dynamic_lds;  // hipFuncSetAttribute
std::vector<std::pair<std::string, std::deque<float>>> g_scripts;
std::vector<std::pair<std::string, fakehip::Effect>> g_effects;
std::vector<Failure> g_failures;
std::map<std::string, uint64_t> g_calls;
uint64_t g_injectable = 0, g_stream_syncs = 0;
std::string g_injected, g_case;
FILE* g_trace = nullptr;
struct CallConfig { dim3 grid, block; size_t lds; hipStream_t stream; };
thread_local std::vector<CallConfig> g_configs;

std::string demangled(const char* name) {
    int status = 0;
    char* d = abi::__cxa_demangle(name, nullptr, nullptr, &status);
    std::string s = (status == 0 && d) ? d : name;
    free(d);
    if (s.compare(0, 5, "void ") == 0) s.erase(0, 5);
    int depth = 0;      // drop the parameter list: the last top-level '('
    for (size_t i = s.size(); i-- > 0;) {
        if (s[i] == ')') ++depth;
        else if (s[i] == '(' && --depth == 0) { s.erase(i); break; }
    }
    return s;
}

// true: the call fails with *e (and counts as made)
bool injected(const char* fn, hipError_t* e) {
    ++g_injectable;
    const uint64_t n = ++g_calls[fn];
    for (size_t i = 0; i < g_failures.size(); ++i) {
        Failure& f = g_failures[i];
        if (f.global ? f.at == g_injectable : (f.fn == fn && f.at == n)) {
            *e = f.e; g_injected = fn;
            g_failures.erase(g_failures.begin() + i);
            return true;
        }
    }
    return false;
}
void count(const char* fn) { ++g_calls[fn]; }

Range* range_of(uintptr_t p) {
    auto it = g_ranges.upper_bound(p);
    if (it == g_ranges.begin()) return nullptr;
    --it;
    Range& r = it->second;
    return (p >= r.base && p < r.base + r.bytes) ? &r : nullptr;
}

// bytes usable from p on: to the end of a live block, or through the chunks mapped side by side with access set
size_t extent_at(uintptr_t p, Range** out = nullptr) {
    Range* r = range_of(p);
    if (out) *out = r;
    if (!r || !r->alive) return 0;
    if (r->kind != fakehip::KIND_RESERVED) return r->base + r->bytes - p;
    size_t at = p - r->base, end = at;
    bool moved = true;
    while (moved) {
        moved = false;
        for (const Mapping& m : r->maps)
            if (m.access && m.off <= end && end < m.off + m.bytes) { end = m.off + m.bytes; moved = true; }
    }
    return end - at;
}

// ---- the stream model ---------------------------------------------------------------------------------------------------------------
std::map<void*, StreamState> g_streams;        // the null stream is g_streams[nullptr]
std::deque<Op> g_pending;                      // entries nothing has completed yet, by id
uint64_t g_op = 0;
std::vector<std::pair<uint64_t, std::string>> g_unordered_ok;      // allow_unordered: `born` of the range, why

StreamState& stream_state(void* s) {
    auto it = g_streams.find(s);
    if (it == g_streams.end()) {
        if (s != nullptr) fakehip::violation("(runtime)", "stream", "a call names a stream that was never created (or is destroyed)");
        it = g_streams.emplace(s, StreamState()).first;
    }
    return it->second;
}
void merge(Clock& into, const Clock& from) { for (const auto& kv : from) { uint64_t& v = into[kv.first]; v = std::max(v, kv.second); } }
void merge(Clock& into, void* s, uint64_t id) { if (id) { uint64_t& v = into[s]; v = std::max(v, id); } }
bool allowed_unordered(uint64_t born) {
    for (const auto& a : g_unordered_ok) if (a.first == born) return true;
    return false;
}
std::string op_name(const Op& p) { return p.what + " (entry " + std::to_string(p.id) + " of stream " + (p.stream ? "0x" + std::to_string((uintptr_t)p.stream % 100000) : std::string("null")) + ")"; }

// a lifetime question: does an entry still in flight reference the range?  On the null stream and on blocking streams only launches
// count, as before there were queues (a copy there is carried out at once); on a non-blocking stream every entry does
bool any_in_flight_on(uint64_t born, std::string* who) {
    for (const Op& p : g_pending) {
        if (p.type != OP_LAUNCH && stream_state(p.stream).kind != fakehip::STREAM_NON_BLOCKING) continue;
        for (const fakehip::Span& s : p.spans) if (s.born == born) { *who = p.type == OP_LAUNCH ? p.what + " (launch " + std::to_string(p.launch_seq) + ")" : op_name(p); return true; }
    }
    return false;
}

// the `order` rule: `spans` of a new entry of `stream` (or of the host: a synchronous copy, a map; host = true) against every entry
// in flight on another stream that no edge puts in front of it
void check_order(const std::string& what, void* stream, bool host, const Clock& clock, const std::vector<fakehip::Span>& spans) {
    if (spans.empty()) return;
    for (const Op& p : g_pending) {
        if (p.spans.empty()) continue;
        if (host) { if (stream_state(p.stream).kind != fakehip::STREAM_NON_BLOCKING) continue; }      // a synchronous call waits for the null stream and the blocking ones itself
        else {
            if (p.stream == stream) continue;
            auto it = clock.find(p.stream);
            if (it != clock.end() && it->second >= p.id) continue;
        }
        for (const fakehip::Span& a : p.spans) for (const fakehip::Span& b : spans) {
            if (a.born != b.born || !(a.write || b.write) || a.lo >= b.hi || b.lo >= a.hi) continue;
            if (allowed_unordered(a.born)) continue;
            fakehip::violation(what, "order", std::string(b.write ? "writes" : "reads") + " " + std::to_string(std::min(a.hi, b.hi) - std::max(a.lo, b.lo)) + " bytes of allocation " + std::to_string(a.born) +
                               " that " + op_name(p) + " " + (a.write ? "writes" : "reads") + ", still in flight, and no event, wait or synchronisation orders the two");
        }
    }
}

// the legacy null stream waits for every blocking stream and every blocking stream for it
void legacy_edges(void* s, StreamState& st) {
    if (st.kind == fakehip::STREAM_NULL) { for (auto& kv : g_streams) if (kv.second.kind == fakehip::STREAM_BLOCKING) { merge(st.clock, kv.first, kv.second.last); merge(st.clock, kv.second.clock); } }
    else if (st.kind == fakehip::STREAM_BLOCKING) { StreamState& n = stream_state(nullptr); merge(st.clock, nullptr, n.last); merge(st.clock, n.clock); }
    (void)s;
}
Op& enqueue(Op op) {
    StreamState& st = stream_state(op.stream);
    legacy_edges(op.stream, st);
    check_order(op.what, op.stream, false, st.clock, op.spans);
    op.id = ++g_op; op.clock = st.clock; st.last = op.id;
    g_pending.push_back(std::move(op));
    return g_pending.back();
}
void finish(Op& p) {
    if (p.deferred) for (size_t i = 0; i < p.height; ++i) std::memcpy((uint8_t*)p.dst + i * p.dpitch, p.staged.data() + i * p.width, p.width);
    if (p.pinned_src && std::memcmp(p.pinned_src, p.pinned_copy.data(), p.pinned_copy.size()) != 0)
        fakehip::violation(p.what, "order", "the page-locked source of " + op_name(p) + " was changed by the host while the copy was in flight");
    if (p.type == OP_LAUNCH) g_launches[p.launch_seq - 1].in_flight = false;
}
// completes the entries `pick` names and whatever they wait for, oldest first
template <class Pick> void complete_where(Pick pick) {
    std::vector<char> take(g_pending.size(), 0);
    bool any = false;
    for (size_t i = 0; i < g_pending.size(); ++i) if (pick(g_pending[i])) { take[i] = 1; any = true; }
    if (!any) return;
    for (bool moved = true; moved;) {
        moved = false;
        Clock need;
        for (size_t i = 0; i < g_pending.size(); ++i) if (take[i]) { merge(need, g_pending[i].clock); merge(need, g_pending[i].stream, g_pending[i].id); }
        for (size_t i = 0; i < g_pending.size(); ++i) {
            if (take[i]) continue;
            auto it = need.find(g_pending[i].stream);
            if (it != need.end() && g_pending[i].id <= it->second) { take[i] = 1; moved = true; }
        }
    }
    std::deque<Op> rest;
    for (size_t i = 0; i < g_pending.size(); ++i) { if (take[i]) finish(g_pending[i]); else rest.push_back(std::move(g_pending[i])); }
    g_pending.swap(rest);
}
void complete_stream(void* s, uint64_t upto) { complete_where([&](const Op& p) { return p.stream == s && p.id <= upto; }); }
// a synchronous hipMemcpy / hipMemset / hipFree: the null stream and every blocking stream, not a non-blocking one
void complete_legacy() { complete_where([&](const Op& p) { return stream_state(p.stream).kind != fakehip::STREAM_NON_BLOCKING; }); }
void span_of(std::vector<fakehip::Span>& out, const void* p, size_t bytes, bool write);

// Under AddressSanitizer the rest of a block's last page is poisoned: the block is exactly as long as it was asked for (in front of it
// and behind the page lies nothing, or another mapping's own checked bytes).
void guard_tail(uintptr_t base, size_t bytes, bool on) {
#ifdef FAKEHIP_ASAN
    const size_t rounded = std::max((bytes + kPage - 1) / kPage * kPage, kPage);
    if (on) ASAN_POISON_MEMORY_REGION((void*)(base + bytes), rounded - bytes);
    else ASAN_UNPOISON_MEMORY_REGION((void*)base, rounded);
#else
    (void)base; (void)bytes; (void)on;
#endif
}
void fresh_fill(uintptr_t base, size_t bytes) { if (g_fresh_fill >= 0) std::memset((void*)base, g_fresh_fill, std::min(bytes, kFillLimit)); }

void* map_pages(size_t bytes, int prot) {
    bytes = (bytes + kPage - 1) / kPage * kPage;
    void* p = mmap(nullptr, std::max(bytes, kPage), prot, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
    if (p == MAP_FAILED) { fprintf(stderr, "fakehip: mmap of %zu bytes failed\n", bytes); abort(); }
    return p;
}

hipError_t new_block(void** ptr, size_t bytes, int kind) {
    if (!ptr) return hipErrorInvalidValue;
    if (bytes == 0) { *ptr = nullptr; return hipSuccess; }
    if (kind != fakehip::KIND_HOST) {
        if (g_live + bytes > g_capacity) return hipErrorOutOfMemory;
        g_live += bytes; g_peak = std::max(g_peak, g_live);
    }
    Range r;
    r.base = (uintptr_t)map_pages(bytes, PROT_READ | PROT_WRITE); r.bytes = bytes; r.kind = kind; r.device = g_device; r.born = ++g_born;
    g_ranges[r.base] = r;
    fresh_fill(r.base, bytes);
    guard_tail(r.base, bytes, true);
    *ptr = (void*)r.base;
    return hipSuccess;
}

hipError_t free_block(void* p, const char* fn, int kind) {
    if (!p) return hipSuccess;
    auto it = g_ranges.find((uintptr_t)p);
    if (it == g_ranges.end() || it->second.kind != kind) fakehip::violation(fn, "pointer", "not the base of a live allocation of that kind");
    Range r = it->second;
    std::string who;
    if (any_in_flight_on(r.born, &who)) fakehip::violation(who, "lifetime", std::string(fn) + " of a range that launch still references (nothing has waited for it)");
    guard_tail(r.base, r.bytes, false);
    munmap((void*)r.base, std::max((r.bytes + kPage - 1) / kPage * kPage, kPage));
    if (kind != fakehip::KIND_HOST) g_live -= r.bytes;
    r.alive = false;
    g_dead.push_back(r);
    g_ranges.erase(it);
    return hipSuccess;
}

// ---- the launch contract -----------------------------------------------------------------------------------------------------
struct Checker {
    fakehip::Launch& l;
    explicit Checker(fakehip::Launch& launch) : l(launch) {}
    [[noreturn]] void bad(const std::string& field, const std::string& what) const { fakehip::violation(l.kernel, field, what); }
    // `bytes` from p lie in one live extent (a null pointer is the caller's business: `optional`)
    void need(const char* field, const void* p, uint64_t bytes, bool optional = false, bool write = true) {
        if (!p) { if (optional) return; bad(field, "null"); }
        Range* r = nullptr;
        const size_t have = extent_at((uintptr_t)p, &r);
        if (!r) bad(field, "points into no allocation (freed, or never made)");
        if (!r->alive) bad(field, "points into a dead range");
        if (have == 0) bad(field, "points into a reserved range with nothing mapped there (or no access set)");
        if (bytes > have) bad(field, "needs " + std::to_string(bytes) + " bytes, the live extent from there holds " + std::to_string(have));
        r->last_launch = l.seq;
        if (std::find(l.refs.begin(), l.refs.end(), r->born) == l.refs.end()) l.refs.push_back(r->born);
        l.spans.push_back({r->born, (uintptr_t)p, (uintptr_t)p + std::max<uint64_t>(bytes, 1), write});
    }
    void ro(const char* field, const void* p, uint64_t bytes, bool optional = false) { need(field, p, bytes, optional, false); }      // the struct declares the pointer const
    // per-stream ranges base + off[s] .. + size[s] (or the uniform layout s * stream_len); the arrays themselves are checked first
    void ranges(const char* field, const uint8_t* base, const uint64_t* off, const uint32_t* sizes, uint32_t n, uint64_t uniform, bool optional = false, bool write = false) {
        if (!base) { if (optional) return; bad(field, "null"); }
        const std::string f = field;
        if (off) { ro((f + "_offsets").c_str(), off, (uint64_t)n * 8u); ro((f + "_sizes").c_str(), sizes, (uint64_t)n * 4u); }
        Range* r = nullptr;
        const size_t have = extent_at((uintptr_t)base, &r);
        if (!r || !r->alive || have == 0) { need(field, base, 1); return; }
        need(field, base, 1, false, write);
        uint64_t lo = ~0ull, hi = 0;
        for (uint32_t s = 0; s < n; ++s) {
            const uint64_t a = off ? off[s] : (uint64_t)s * uniform, b = off ? sizes[s] : uniform;
            if (a + b > have || a + b < a) bad(f + "_offsets[" + std::to_string(s) + "] + " + f + "_sizes", "the stream's range ends at " + std::to_string(a + b) + ", the live extent holds " + std::to_string(have));
            if (b) { lo = std::min(lo, a); hi = std::max(hi, a + b); }
        }
        if (hi > lo) l.spans.push_back({r->born, (uintptr_t)base + lo, (uintptr_t)base + hi, write});      // what the streams of this launch cover, not the whole block
    }
    void seg_list(const uint32_t* seg_begin, const void* segs, uint32_t n, const char* begin_name, const char* list_name, size_t record) {
        if (!seg_begin && !segs) return;
        ro(begin_name, seg_begin, ((uint64_t)n + 1u) * 4u);
        const uint64_t last = seg_begin[n];
        if (last) ro(list_name, segs, last * record); else ro(list_name, segs, 1);
    }
    void lds_rules(const void* fn, bool persistent) {
        auto it = g_max_dynamic_lds.find(fn);
        const uint32_t allowed = it == g_max_dynamic_lds.end() ? 65536u : (uint32_t)it->second;
        if (l.lds > allowed) bad("dynamic LDS", std::to_string(l.lds) + " bytes, hipFuncSetAttribute allowed " + std::to_string(allowed));
        if (l.lds > kLdsPerCu) bad("dynamic LDS", std::to_string(l.lds) + " bytes is more than a CU has");
        if (persistent) {
            const uint64_t per_cu = ((uint64_t)l.grid + kNumCus - 1) / kNumCus;
            if (per_cu * l.lds > kLdsPerCu) bad("dynamic LDS", std::to_string(per_cu) + " workgroups per CU x " + std::to_string(l.lds) + " bytes exceed 160 KiB");
        }
    }
    void tables(const LitBatch& b) {
        const uint64_t slab = (uint64_t)b.geom.total_rows * 32u;
        // lit_decode2.hip:468-475: a workgroup's 16 slabs behind one buffer resource, offsets formed in 32 bits
        if (16u * slab >= ((uint64_t)1 << 31)) bad("geom.total_rows", "16 * slab = " + std::to_string(16u * slab) + " does not fit the 32-bit table offsets");
        need("tables", b.tables, (uint64_t)l.grid * 16u * slab);
        Range* r = range_of((uintptr_t)b.tables);
        l.tables = (uintptr_t)b.tables; l.tables_kind = r->kind == fakehip::KIND_RESERVED ? fakehip::KIND_CHUNK : r->kind; l.tables_born = r->born;
    }
    void lit(const LitBatch& b, const LitCommandLists* cl) {
        const uint32_t n = b.n_streams;
        l.n_streams = n;
        const bool encode = l.kernel.find("lit_model_encode_kernel") != std::string::npos, replay = l.kernel.find("row_replay") != std::string::npos;
        if (l.block != (uint32_t)LIT_THREADS) bad("block", "the streaming kernels run 256 threads");
        ro("blob", b.blob, (uint64_t)b.geom.mix_off + 8192u);
        tables(b);
        if (!replay) need("status", b.status, 4);
        ranges("in", b.in, b.in_offsets, b.in_sizes, n, b.stream_len);
        if (!b.in_offsets && !encode && !replay) bad("in_offsets", "the decoders take coded streams by offset and size");
        if (encode) need("sf", b.sf, (uint64_t)n * 2u * b.max_stream_len * 4u);
        else if (!replay) ranges("out", b.out, b.out_offsets, b.out_sizes, n, b.stream_len, false, true);
        need("stream_bad", b.stream_bad, n, true);
        ro("byte_rank", b.byte_rank, 256, true);
        need("consumed", b.consumed, (uint64_t)n * 4u, true);
        if (b.resume || b.wstate) need("wstate", b.wstate, 24);
        seg_list(b.seg_begin, b.segs, n, "seg_begin", "segs", sizeof(LitSegment));
        if (cl) {
            seg_list(cl->cmd_begin, cl->cmds, n, "cmd_begin", "cmds", sizeof(LitCommand));
            ro("lit_sizes", cl->lit_sizes, (uint64_t)n * 4u);
            ranges("ins", cl->ins, cl->ins_offsets, cl->ins_sizes, n, 0, true);
            ranges("hist", cl->hist, cl->hist_offsets, cl->hist_sizes, n, 0, true);
        }
    }
    void rans(const RansBatch& b) {
        const uint32_t n = b.n_streams;
        l.n_streams = n;
        if (b.sf_stride % 4u) bad("sf_stride", "not a multiple of 4");
        ro("sf", b.sf, (uint64_t)n * b.sf_stride * 4u);
        ro("in_sizes", b.in_sizes, (uint64_t)n * 4u, true);
        need("out", b.out, (uint64_t)n * b.out_slot);
        need("out_offsets", b.out_offsets, (uint64_t)n * 8u);
        need("out_sizes", b.out_sizes, (uint64_t)n * 4u);
        need("status", b.status, 4);
        if (b.chunk_bytes) need("chunk_bytes", b.chunk_bytes, (uint64_t)n * b.max_chunks * 4u);
        if (b.scratch) { need("scratch", b.scratch, (uint64_t)n * b.scratch_stride); need("chunk0_sizes", b.chunk0_sizes, (uint64_t)n * 4u); }
    }
    template <class B> void bucket_common(const B& b) {
        const uint64_t n = b.n_streams;
        l.n_streams = b.n_streams;
        if (b.pieces == 0 || b.pieces > 8u || b.slot < b.pieces * 8192u) bad("pieces / slot", "a slot is `pieces` (1..8) pieces of 8192 elements");
        if (n * 256u >= ((uint64_t)1 << 32)) bad("n_streams", "task ids stream * 256 + key leave 32 bits");
        ranges("in", b.in, b.in_offsets, b.in_sizes, b.n_streams, b.stream_len);
        need("inv", b.inv, n * b.slot * 2u);
        need("desc", b.desc, n * 256u * 8u * 4u);
        need("tasks", b.tasks, 6u * n * 256u * 4u);
        need("counters", b.counters, 64);
        seg_list(b.seg_begin, b.segs, b.n_streams, "seg_begin", "segs", sizeof(LitSegment));
    }
    // The kernels of lit_bucket.hip also serve the other passes, which hand them a view with the fields they do not read null
    // (lit_bucket_mix.hip:433, lit_bucket_ctx.hip:219): what a kernel reads or writes is required, the rest is checked where it is set.
    void bucket(const BucketBatch& b) {
        bucket_common(b);
        const uint64_t n = b.n_streams;
        const bool sort = has_name("bucket_sort"), chain = has_name("bucket_chain"), unsort32 = has_name("bucket_unsort32"), unsort = !unsort32 && has_name("bucket_unsort");
        need("sorted", b.sorted, n * b.slot, !(sort || chain));
        need("sfs", b.sfs, n * b.slot * (unsort32 ? 4u : 8u), !(chain || unsort || unsort32));
        need("sf", b.sf, n * b.sf_stride * 4u, !(unsort || unsort32));
        need("status", b.status, 4, !sort);
    }
    bool has_name(const char* what) const { return l.kernel.find(what) != std::string::npos; }
    void mix(const MixBucketBatch& b) {
        bucket_common(b);
        const uint64_t n = b.n_streams;
        const bool one_model = b.xs[1] == nullptr;      // the context-keyed one-model pass: byte payloads, one plane
        need("sf", b.sf, n * b.sf_stride * 4u);
        need("status", b.status, 4);
        ro("blob", b.blob, 256u + 2048u * (uint64_t)std::max(b.n_btypes, 1u));
        need("sorted", b.sorted, n * b.slot * (one_model ? 1u : 2u));
        need("xs[0]", b.xs[0], n * b.pos_stride * 8u);
        if (!one_model) {
            need("xs[1]", b.xs[1], n * b.pos_stride * 8u);
            need("maxes[0]", b.maxes[0], n * b.pos_stride * 4u);
            need("maxes[1]", b.maxes[1], n * b.pos_stride * 4u);
        }
    }
    void prepare(const LitCommandPrepare& b) {
        const uint32_t n = b.n_streams;
        l.n_streams = n;
        ranges("raw", b.raw, b.raw_offsets, b.raw_sizes, n, 0);
        if (!b.raw_offsets) bad("raw_offsets", "null");
        seg_list(b.cmd_begin, b.cmds, n, "cmd_begin", "cmds", sizeof(LitCommand));
        if (b.cmd_begin[0] != b.cmd_first || b.cmd_begin[n] != b.cmd_last) bad("cmd_first / cmd_last", "not the ends of cmd_begin");
        ranges("ins", b.ins, b.ins_offsets, b.ins_sizes, n, 0, true);
        ranges("hist", b.hist, b.hist_offsets, b.hist_sizes, n, 0, true);
        if (b.lit_slot % 16u || b.lit_slot < b.lit_stream_len) bad("lit_slot", "lit_stream_len rounded up to 16 bytes");
        need("lit", b.lit, (uint64_t)n * b.lit_slot);
        need("lit_offsets", b.lit_offsets, (uint64_t)n * 8u);
        need("lit_sizes", b.lit_sizes, (uint64_t)n * 4u);
        need("seg_begin", b.seg_begin, ((uint64_t)n + 1u) * 4u);
        need("segs", b.segs, std::max<uint64_t>(b.cmd_last - b.cmd_first, 1u) * sizeof(LitSegment));
        need("out_lit_sizes", b.out_lit_sizes, (uint64_t)n * 4u);
        need("status", b.status, 4);
        need("stream_bad", b.stream_bad, n, true);
    }
};

bool has(const std::string& s, const char* what) { return s.find(what) != std::string::npos; }

void check_launch(fakehip::Launch& l, const void* fn, void** args) {
    Checker c(l);
    const std::string& k = l.kernel;
    auto keep = [&](const void* p, size_t bytes) { l.args.assign((const uint8_t*)p, (const uint8_t*)p + bytes); };
    if (has(k, "selftest")) { c.lds_rules(fn, false); return; }
    if (has(k, "lit_model_encode_kernel") || has(k, "lit_decode_kernel") || has(k, "lit_decode2_kernel") || has(k, "row_replay_kernel") || has(k, "lit_decode_t_kernel")) {
        keep(args[0], sizeof(LitBatch)); c.lds_rules(fn, true); c.lit(*(const LitBatch*)args[0], nullptr);
    } else if (has(k, "lit_decode2_cmd")) {
        keep(args[0], sizeof(LitBatch)); c.lds_rules(fn, true); c.lit(*(const LitBatch*)args[0], (const LitCommandLists*)args[1]);
    } else if (has(k, "rans_")) {
        keep(args[0], sizeof(RansBatch)); c.lds_rules(fn, false); c.rans(*(const RansBatch*)args[0]);
    } else if (has(k, "bucket_")) {
        keep(args[0], sizeof(BucketBatch)); c.lds_rules(fn, false); c.bucket(*(const BucketBatch*)args[0]);
    } else if (has(k, "ctx_sort_kernel") || has(k, "mix_")) {
        keep(args[0], sizeof(MixBucketBatch)); c.lds_rules(fn, false); c.mix(*(const MixBucketBatch*)args[0]);
    } else if (has(k, "lit_commands_")) {
        keep(args[0], sizeof(LitCommandPrepare)); c.lds_rules(fn, false); c.prepare(*(const LitCommandPrepare*)args[0]);
    } else if (has(k, "scan_sizes_kernel")) {
        const uint32_t n = *(const uint32_t*)args[1];
        l.n_streams = n; c.lds_rules(fn, false);
        const fakehip::ScanArgs sa = {*(const uint32_t**)args[0], n, *(uint64_t**)args[2], *(uint64_t**)args[3], *(const int*)args[4]};
        keep(&sa, sizeof(sa));
        c.ro("sizes", *(const void**)args[0], (uint64_t)n * 4u); c.need("offsets", *(const void**)args[2], (uint64_t)n * 8u); c.need("total", *(const void**)args[3], 8);
    } else if (has(k, "pack_copy_kernel")) {
        const uint32_t n = *(const uint32_t*)args[3];
        l.n_streams = n; c.lds_rules(fn, false);
        const fakehip::PackArgs pa = {*(const uint8_t**)args[0], *(const uint64_t**)args[1], *(const uint32_t**)args[2], n, *(uint8_t**)args[4], *(const uint64_t**)args[5], *(const uint64_t*)args[6], *(uint32_t**)args[7]};
        keep(&pa, sizeof(pa));
        c.ranges("slots", *(const uint8_t**)args[0], *(const uint64_t**)args[1], *(const uint32_t**)args[2], n, 0);
        c.need("packed", *(const void**)args[4], 1); c.ro("dst_off", *(const void**)args[5], (uint64_t)n * 8u); c.need("status", *(const void**)args[7], 4, true);
    } else if (has(k, "learn_byte_rank_kernel")) {
        const uint32_t n = *(const uint32_t*)args[3];
        l.n_streams = n; c.lds_rules(fn, false);
        c.ranges("data", *(const uint8_t**)args[0], *(const uint64_t**)args[1], *(const uint32_t**)args[2], n, *(const uint32_t*)args[4]);
        c.need("rank", *(const void**)args[7], 256);
    } else {
        c.bad("kernel", "no contract is written for this kernel family (tests/c/README.md: how to add one)");
    }
}

const char* kind_name(int k) { return k == fakehip::KIND_BLOCK ? "block" : k == fakehip::KIND_CHUNK ? "chunks" : k == fakehip::KIND_HOST ? "host" : "none"; }

}  // namespace

// ---- the driver's side -------------------------------------------------------------------------------------------------------
namespace fakehip {

void violation(const std::string& kernel, const std::string& field, const std::string& what) {
    fflush(stdout);
    fprintf(stderr, "CONTRACT VIOLATION [%s] kernel %s: field %s: %s\n", g_case.c_str(), kernel.c_str(), field.c_str(), what.c_str());
    if (g_trace) fflush(g_trace);
    abort();
}
void set_capacity(size_t bytes) { g_capacity = bytes; }
void set_fresh_fill(int byte) { g_fresh_fill = byte < 0 ? -1 : (byte & 0xff); }
size_t live_bytes() { return g_live; }
size_t reserved_bytes() { return g_reserved; }
size_t peak_live_bytes() { return g_peak; }
void reset_peak() { g_peak = g_live; }
void script_times(const char* match, const std::vector<float>& ms) { g_scripts.emplace_back(match, std::deque<float>(ms.begin(), ms.end())); }
void fail_call(const char* function, uint64_t kth, hipError_t e) { g_failures.push_back({function, g_calls[function] + kth, e, false}); }
void fail_at(uint64_t index, hipError_t e) { g_failures.push_back({"", g_injectable + index, e, true}); }
uint64_t injectable_calls() { return g_injectable; }
const char* injected_function() { return g_injected.c_str(); }
void clear_failures() { g_failures.clear(); g_injected.clear(); }
void set_effect(const char* match, Effect fn) { g_effects.emplace_back(match, fn); }
void set_case(const char* label) { g_case = label; }
void open_trace(const char* path) { g_trace = fopen(path, "w"); if (!g_trace) { perror(path); abort(); } }
void trace_note(const std::string& body) { if (g_trace) fprintf(g_trace, "{\"note\": true, \"case\": \"%s\", %s}\n", g_case.c_str(), body.c_str()); }
const std::vector<Launch>& launches() { return g_launches; }
int stream_kind(void* stream) { LOCK; auto it = g_streams.find(stream); return it == g_streams.end() ? (stream ? -1 : (int)STREAM_NULL) : it->second.kind; }
size_t pending_entries(void* stream) { LOCK; size_t n = 0; for (const Op& p : g_pending) n += p.stream == stream; return n; }
void allow_unordered(const void* inside_range, const char* why) {
    LOCK;
    Range* r = range_of((uintptr_t)inside_range);
    if (!r) violation("(driver)", "allow_unordered", "the address lies in no ledger range");
    g_unordered_ok.emplace_back(r->born, why);
}
uint64_t stream_syncs() { return g_stream_syncs; }
uint64_t count_calls(const char* function) { return g_calls[function]; }
std::vector<LedgerEntry> ledger() {
    std::vector<LedgerEntry> out;
    for (const auto& kv : g_ranges) {
        const Range& r = kv.second;
        out.push_back({r.base, r.bytes, r.kind, r.device, r.alive, r.last_launch, r.born});
        for (const Mapping& m : r.maps) out.push_back({r.base + m.off, m.bytes, KIND_CHUNK, r.device, true, r.last_launch, r.born});
    }
    for (const Range& r : g_dead) out.push_back({r.base, r.bytes, r.kind, r.device, false, r.last_launch, r.born});
    return out;
}
void check_clean_end() {
    for (const auto& kv : g_ranges) {
        const Range& r = kv.second;
        if (r.kind != KIND_RESERVED) violation("(clean end)", "ledger", std::string("a live ") + kind_name(r.kind) + " of " + std::to_string(r.bytes) + " bytes is left (allocation " + std::to_string(r.born) + ")");
        if (!r.maps.empty()) violation("(clean end)", "ledger", "a reserved range still has " + std::to_string(r.maps.size()) + " chunks mapped");
    }
    for (const auto& kv : g_phys) if (!kv.second.released || kv.second.mapped) violation("(clean end)", "ledger", "a physical chunk was never released");
    if (g_live != 0) violation("(clean end)", "ledger", std::to_string(g_live) + " bytes of device memory are still accounted for");
}

}  // namespace fakehip

// ---- the runtime ---------------------------------------------------------------------------------------------------------------

extern "C" {

hipError_t __hipPushCallConfiguration(dim3 grid, dim3 block, size_t lds, hipStream_t stream) { g_configs.push_back({grid, block, lds, stream}); return hipSuccess; }
hipError_t __hipPopCallConfiguration(dim3* grid, dim3* block, size_t* lds, hipStream_t* stream) {
    if (g_configs.empty()) abort();
    const CallConfig c = g_configs.back(); g_configs.pop_back();
    *grid = c.grid; *block = c.block; *lds = c.lds; *stream = c.stream;
    return hipSuccess;
}
void** __hipRegisterFatBinary(const void*) { static void* handle; return &handle; }
void __hipUnregisterFatBinary(void**) {}
void __hipRegisterFunction(void**, const void* host_fn, char*, const char* device_name, unsigned, void*, void*, void*, void*, int*) {
    kernels()[host_fn] = demangled(device_name);
}
void __hipRegisterVar(void**, void*, char*, const char*, int, size_t, int, int) {}

}  // extern "C"

const char* hipGetErrorString(hipError_t e) {
    switch (e) {
    case hipSuccess: return "no error";
    case hipErrorOutOfMemory: return "out of memory";
    case hipErrorInvalidValue: return "invalid argument";
    case hipErrorLaunchFailure: return "unspecified launch failure";
    case hipErrorNotReady: return "device not ready";
    default: return "fakehip: injected error";
    }
}
hipError_t hipGetLastError(void) { const hipError_t e = g_last_error; g_last_error = hipSuccess; return e; }
hipError_t hipGetDeviceCount(int* n) { *n = 1; return hipSuccess; }
hipError_t hipSetDevice(int d) { if (d != 0) return hipErrorInvalidDevice; g_device = d; return hipSuccess; }
hipError_t hipGetDevice(int* d) { *d = g_device; return hipSuccess; }
hipError_t hipGetDeviceProperties(hipDeviceProp_t* p, int) {      // (the header names this symbol hipGetDevicePropertiesR0600)
    std::memset(p, 0, sizeof(*p));
    snprintf(p->name, sizeof(p->name), "fakehip MI355X");
    snprintf(p->gcnArchName, sizeof(p->gcnArchName), "gfx950:sramecc+:xnack-");
    p->multiProcessorCount = kNumCus; p->warpSize = 64; p->maxThreadsPerBlock = 1024;
    p->sharedMemPerBlock = 65536; p->maxSharedMemoryPerMultiProcessor = kLdsPerCu; p->totalGlobalMem = g_capacity;
    return hipSuccess;
}
hipError_t hipMemGetInfo(size_t* free_b, size_t* total) { LOCK; *total = g_capacity; *free_b = g_capacity > g_live ? g_capacity - g_live : 0; return hipSuccess; }

hipError_t hipMalloc(void** p, size_t bytes) {
    LOCK; hipError_t e;
    if (injected("hipMalloc", &e)) { g_last_error = e; return e; }
    e = new_block(p, bytes, fakehip::KIND_BLOCK);
    if (e != hipSuccess) g_last_error = e;
    return e;
}
hipError_t hipExtMallocWithFlags(void** p, size_t bytes, unsigned) { LOCK; count("hipExtMallocWithFlags"); return new_block(p, bytes, fakehip::KIND_BLOCK); }
hipError_t hipFree(void* p) { LOCK; count("hipFree"); return free_block(p, "hipFree", fakehip::KIND_BLOCK); }      // completes nothing: a free under a launch stays a violation
hipError_t hipHostMalloc(void** p, size_t bytes, unsigned) { LOCK; count("hipHostMalloc"); return new_block(p, bytes, fakehip::KIND_HOST); }
hipError_t hipHostFree(void* p) { LOCK; count("hipHostFree"); return free_block(p, "hipHostFree", fakehip::KIND_HOST); }

// ---- virtual memory management
hipError_t hipMemGetAllocationGranularity(size_t* g, const hipMemAllocationProp*, hipMemAllocationGranularity_flags) { *g = kGranularity; return hipSuccess; }
hipError_t hipMemAddressReserve(void** p, size_t bytes, size_t, void*, unsigned long long) {
    LOCK; hipError_t e;
    if (injected("hipMemAddressReserve", &e)) { g_last_error = e; return e; }
    if (bytes == 0 || bytes % kGranularity) return hipErrorInvalidValue;
    Range r;
    r.base = (uintptr_t)map_pages(bytes, PROT_NONE); r.bytes = bytes; r.kind = fakehip::KIND_RESERVED; r.device = g_device; r.born = ++g_born;
    g_ranges[r.base] = r; g_reserved += bytes;
    *p = (void*)r.base;
    return hipSuccess;
}
hipError_t hipMemAddressFree(void*, size_t) {
    fakehip::violation("(runtime)", "hipMemAddressFree", "an address range is never handed back (divans_amd/csrc/capi.cpp, the remap defect)");
}
hipError_t hipMemCreate(hipMemGenericAllocationHandle_t* h, size_t bytes, const hipMemAllocationProp* prop, unsigned long long) {
    LOCK; hipError_t e;
    if (injected("hipMemCreate", &e)) { g_last_error = e; return e; }
    if (bytes == 0 || bytes % kGranularity) return hipErrorInvalidValue;
    if (g_live + bytes > g_capacity) { g_last_error = hipErrorOutOfMemory; return hipErrorOutOfMemory; }
    g_live += bytes; g_peak = std::max(g_peak, g_live);
    const uint64_t id = g_next_handle++;
    g_phys[id] = {bytes, prop ? prop->location.id : 0, false, 0};
    *h = (hipMemGenericAllocationHandle_t)(uintptr_t)id;
    return hipSuccess;
}
static void phys_gone_if_unused(uint64_t id) {
    auto it = g_phys.find(id);
    if (it != g_phys.end() && it->second.released && it->second.mapped == 0) { g_live -= it->second.bytes; g_phys.erase(it); }
}
hipError_t hipMemRelease(hipMemGenericAllocationHandle_t h) {
    LOCK; count("hipMemRelease");
    auto it = g_phys.find((uint64_t)(uintptr_t)h);
    if (it == g_phys.end() || it->second.released) fakehip::violation("(runtime)", "hipMemRelease", "not a live handle");
    it->second.released = true;
    phys_gone_if_unused(it->first);
    return hipSuccess;
}
hipError_t hipMemMap(void* p, size_t bytes, size_t offset, hipMemGenericAllocationHandle_t h, unsigned long long) {
    LOCK; hipError_t e;
    if (injected("hipMemMap", &e)) { g_last_error = e; return e; }
    Range* r = range_of((uintptr_t)p);
    auto ph = g_phys.find((uint64_t)(uintptr_t)h);
    if (!r || r->kind != fakehip::KIND_RESERVED || ph == g_phys.end() || offset != 0 || bytes != ph->second.bytes || (uintptr_t)p + bytes > r->base + r->bytes) return hipErrorInvalidValue;
    if (r->sealed && !r->maps.empty()) fakehip::violation("(runtime)", "hipMemMap", "a chunk is mapped into a range while part of an earlier mapping is still there");
    { std::string who; if (any_in_flight_on(r->born, &who)) fakehip::violation(who, "order", "hipMemMap into a range that entry still references (nothing has waited for it)"); }
    const size_t off = (uintptr_t)p - r->base;
    for (const Mapping& m : r->maps) if (off < m.off + m.bytes && m.off < off + bytes) fakehip::violation("(runtime)", "hipMemMap", "the addresses are mapped already");
    r->sealed = false;
    r->maps.push_back({off, bytes, ph->first, false});
    ++ph->second.mapped;
    return hipSuccess;
}
hipError_t hipMemSetAccess(void* p, size_t bytes, const hipMemAccessDesc*, size_t) {
    LOCK; count("hipMemSetAccess");
    Range* r = range_of((uintptr_t)p);
    if (!r || r->kind != fakehip::KIND_RESERVED) return hipErrorInvalidValue;
    const size_t off = (uintptr_t)p - r->base;
    for (Mapping& m : r->maps) if (m.off >= off && m.off + m.bytes <= off + bytes) {
        const bool fresh = !m.access;
        m.access = true;
        mprotect((void*)(r->base + m.off), m.bytes, PROT_READ | PROT_WRITE);
        if (fresh) fresh_fill(r->base + m.off, m.bytes);
    }
    r->sealed = true;
    return hipSuccess;
}
hipError_t hipMemUnmap(void* p, size_t bytes) {
    LOCK; count("hipMemUnmap");
    Range* r = range_of((uintptr_t)p);
    if (!r || r->kind != fakehip::KIND_RESERVED) fakehip::violation("(runtime)", "hipMemUnmap", "not inside a reserved range");
    const size_t off = (uintptr_t)p - r->base;
    for (size_t i = 0; i < r->maps.size(); ++i) {
        if (r->maps[i].off != off || r->maps[i].bytes != bytes) continue;
        std::string who;
        if (any_in_flight_on(r->born, &who)) fakehip::violation(who, "lifetime", "hipMemUnmap inside a range that launch still references (nothing has waited for it)");
        madvise((void*)(r->base + off), bytes, MADV_DONTNEED);
        mprotect((void*)(r->base + off), bytes, PROT_NONE);
        const uint64_t id = r->maps[i].handle;
        r->maps.erase(r->maps.begin() + i);
        --g_phys[id].mapped;
        phys_gone_if_unused(id);
        if (r->maps.empty()) r->sealed = false;
        return hipSuccess;
    }
    fakehip::violation("(runtime)", "hipMemUnmap", "no chunk is mapped at exactly that place");
}

// ---- copies and fills: carried out where the host reads or writes, checked everywhere
static void check_device_side(const char* fn, const char* field, const void* p, size_t bytes) {
    if (bytes == 0) return;
    Range* r = nullptr;
    const size_t have = extent_at((uintptr_t)p, &r);
    if (!r) return;     // ordinary host memory
    if (have < bytes) fakehip::violation(fn, field, "needs " + std::to_string(bytes) + " bytes, the live extent from there holds " + std::to_string(have));
}
namespace {
void span_of(std::vector<fakehip::Span>& out, const void* p, size_t bytes, bool write) {
    if (bytes == 0) return;
    Range* r = range_of((uintptr_t)p);
    if (r) out.push_back({r->born, (uintptr_t)p, (uintptr_t)p + bytes, write});
}
bool device_side(const void* p) { Range* r = range_of((uintptr_t)p); return r && r->kind != fakehip::KIND_HOST; }
}
// One copy of `height` rows of `width` bytes.  sync: hipMemcpy (waits for the null stream and the blocking ones; an entry of a
// non-blocking stream that touches the same bytes is an `order` violation).  Otherwise an entry of `stream`'s queue: device memory
// is written at once, in program order; on a non-blocking stream a destination in host memory receives the bytes -- as they are
// at this place of the queue -- when the entry completes, and a page-locked source must keep its bytes until then.
static hipError_t copy_rows(const char* fn, void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t height, hipMemcpyKind kind, bool sync, hipStream_t stream) {
    LOCK; count(fn);
    if (width == 0 || height == 0) return hipSuccess;
    const size_t dbytes = (height - 1) * dpitch + width, sbytes = (height - 1) * spitch + width;
    check_device_side(fn, "dst", dst, dbytes); check_device_side(fn, "src", src, sbytes);
    Op op; op.stream = stream; op.type = OP_COPY; op.what = fn;
    span_of(op.spans, dst, dbytes, true); span_of(op.spans, src, sbytes, false);
    const bool carry = kind != hipMemcpyDeviceToDevice || width * height <= kCopyLimit;
    auto carry_out = [&]() { if (carry) for (size_t i = 0; i < height; ++i) std::memmove((uint8_t*)dst + i * dpitch, (const uint8_t*)src + i * spitch, width); };
    if (sync) {
        check_order(fn, nullptr, true, Clock(), op.spans);
        complete_legacy();
        carry_out();
        return hipSuccess;
    }
    const bool non_blocking = stream_state(stream).kind == fakehip::STREAM_NON_BLOCKING;
    if (non_blocking && !device_side(dst)) {
        op.deferred = true; op.dst = dst; op.dpitch = dpitch; op.width = width; op.height = height;
        op.staged.resize(width * height);
        for (size_t i = 0; i < height; ++i) std::memcpy(op.staged.data() + i * width, (const uint8_t*)src + i * spitch, width);
    } else carry_out();
    Range* sr = range_of((uintptr_t)src);
    if (non_blocking && sr && sr->kind == fakehip::KIND_HOST && height == 1 && width <= kCopyLimit) { op.pinned_src = src; op.pinned_copy.assign((const uint8_t*)src, (const uint8_t*)src + width); }
    enqueue(std::move(op));
    return hipSuccess;
}
hipError_t hipMemcpy(void* dst, const void* src, size_t bytes, hipMemcpyKind kind) { return copy_rows("hipMemcpy", dst, bytes, src, bytes, bytes, 1, kind, true, nullptr); }
hipError_t hipMemcpyAsync(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t s) { return copy_rows("hipMemcpyAsync", dst, bytes, src, bytes, bytes, 1, kind, false, s); }
hipError_t hipMemcpy2DAsync(void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t height, hipMemcpyKind kind, hipStream_t s) {
    if (height == 0 || width == 0) { LOCK; count("hipMemcpy2DAsync"); return hipSuccess; }
    if (width > dpitch || width > spitch) { LOCK; count("hipMemcpy2DAsync"); return hipErrorInvalidPitchValue; }
    return copy_rows("hipMemcpy2DAsync", dst, dpitch, src, spitch, width, height, kind, false, s);
}
static hipError_t fill_impl(const char* fn, void* p, int v, size_t bytes, bool sync, hipStream_t stream) {
    LOCK; count(fn);
    check_device_side(fn, "dst", p, bytes);
    Op op; op.stream = stream; op.type = OP_FILL; op.what = fn;
    span_of(op.spans, p, bytes, true);
    if (sync) { check_order(fn, nullptr, true, Clock(), op.spans); complete_legacy(); }
    if (v == 0 && bytes >= ((size_t)1 << 20)) {      // whole pages go back to the zero page, the ends are written
        const uintptr_t a = (uintptr_t)p, lo = (a + kPage - 1) / kPage * kPage, hi = (a + bytes) / kPage * kPage;
        std::memset(p, 0, lo - a); madvise((void*)lo, hi - lo, MADV_DONTNEED); std::memset((void*)hi, 0, a + bytes - hi);
    } else std::memset(p, v, bytes);
    if (!sync) enqueue(std::move(op));
    return hipSuccess;
}
hipError_t hipMemset(void* p, int v, size_t bytes) { return fill_impl("hipMemset", p, v, bytes, true, nullptr); }
hipError_t hipMemsetAsync(void* p, int v, size_t bytes, hipStream_t s) { return fill_impl("hipMemsetAsync", p, v, bytes, false, s); }

// ---- streams and events
hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned flags) {
    LOCK; count("hipStreamCreateWithFlags");
    *s = (hipStream_t) new int(0);
    StreamState st; st.kind = (flags & hipStreamNonBlocking) ? fakehip::STREAM_NON_BLOCKING : fakehip::STREAM_BLOCKING;
    g_streams[(void*)*s] = st;
    return hipSuccess;
}
hipError_t hipStreamCreate(hipStream_t* s) { return hipStreamCreateWithFlags(s, hipStreamDefault); }
hipError_t hipStreamGetFlags(hipStream_t s, unsigned* flags) { LOCK; count("hipStreamGetFlags"); *flags = stream_state(s).kind == fakehip::STREAM_NON_BLOCKING ? hipStreamNonBlocking : hipStreamDefault; return hipSuccess; }
hipError_t hipStreamDestroy(hipStream_t s) {      // the real call lets the queue run out and returns at once; nobody can name the stream afterwards, so the queue is completed here
    LOCK; count("hipStreamDestroy");
    if (!s || !g_streams.count((void*)s)) fakehip::violation("(runtime)", "hipStreamDestroy", "not a live stream");
    complete_stream(s, ~0ull);
    g_streams.erase((void*)s);
    delete (int*)s;
    return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t s) { LOCK; count("hipStreamSynchronize"); ++g_stream_syncs; (void)stream_state(s); complete_stream(s, ~0ull); return hipSuccess; }
hipError_t hipDeviceSynchronize(void) { LOCK; count("hipDeviceSynchronize"); complete_where([](const Op&) { return true; }); return hipSuccess; }
hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t e, unsigned) {
    LOCK; count("hipStreamWaitEvent");
    Event* ev = (Event*)e;
    if (!ev->recorded) return hipSuccess;      // as the real call: an event never recorded orders nothing
    StreamState& st = stream_state(s);
    merge(st.clock, ev->clock);
    Op op; op.stream = s; op.type = OP_WAIT; op.what = "hipStreamWaitEvent";
    enqueue(std::move(op));
    return hipSuccess;
}
hipError_t hipEventCreate(hipEvent_t* e) { LOCK; count("hipEventCreate"); *e = (hipEvent_t) new Event(); return hipSuccess; }
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) { return hipEventCreate(e); }
hipError_t hipEventDestroy(hipEvent_t e) { LOCK; count("hipEventDestroy"); delete (Event*)e; return hipSuccess; }
hipError_t hipEventRecord(hipEvent_t e, hipStream_t s) {
    LOCK; hipError_t err;
    if (injected("hipEventRecord", &err)) { g_last_error = err; return err; }
    Event* ev = (Event*)e;
    Op op; op.stream = s; op.type = OP_RECORD; op.what = "hipEventRecord";
    const Op& q = enqueue(std::move(op));
    ev->stream = s; ev->recorded = true; ev->seq = g_launches.size();      // behind every launch made so far
    ev->id = q.id; ev->clock = q.clock; merge(ev->clock, s, q.id);
    return hipSuccess;
}
hipError_t hipEventSynchronize(hipEvent_t e) {
    LOCK; hipError_t err;
    if (injected("hipEventSynchronize", &err)) { g_last_error = err; return err; }
    Event* ev = (Event*)e;
    if (ev->recorded) complete_stream(ev->stream, ev->id);
    return hipSuccess;
}
hipError_t hipEventQuery(hipEvent_t e) {
    LOCK; count("hipEventQuery");
    Event* ev = (Event*)e;
    if (ev->recorded) for (const Op& p : g_pending) if (p.stream == ev->stream && p.id <= ev->id) return hipErrorNotReady;
    return hipSuccess;
}
hipError_t hipEventElapsedTime(float* ms, hipEvent_t a, hipEvent_t b) {
    LOCK; count("hipEventElapsedTime");
    Event *e0 = (Event*)a, *e1 = (Event*)b;
    if (!e0->recorded || !e1->recorded) return hipErrorInvalidHandle;
    float t = 0.f;
    for (const fakehip::Launch& l : g_launches) {
        if (l.stream != e1->stream || l.seq > e1->seq) continue;
        if (l.in_flight) return hipErrorNotReady;
        if (l.seq > e0->seq) t += g_durations[l.seq - 1];
    }
    *ms = t;
    return hipSuccess;
}
// ---- launches
hipError_t hipFuncSetAttribute(const void* fn, hipFuncAttribute attr, int value) {
    LOCK; count("hipFuncSetAttribute");
    if (attr == hipFuncAttributeMaxDynamicSharedMemorySize) g_max_dynamic_lds[fn] = value;
    return hipSuccess;
}
hipError_t hipLaunchKernel(const void* fn, dim3 grid, dim3 block, void** args, size_t lds, hipStream_t stream) {
    LOCK; hipError_t e;
    if (injected("hipLaunchKernel", &e)) { g_last_error = e; return e; }
    auto it = kernels().find(fn);
    if (it == kernels().end()) fakehip::violation("(unknown)", "function", "hipLaunchKernel of a stub that was never registered");
    if (grid.x == 0 || grid.y != 1 || grid.z != 1 || block.x == 0 || block.x > 1024 || block.y != 1 || block.z != 1) { g_last_error = hipErrorInvalidConfiguration; return g_last_error; }
    fakehip::Launch l;
    l.seq = g_launches.size() + 1; l.kernel = it->second; l.label = g_case;
    l.grid = grid.x; l.block = block.x; l.lds = (uint32_t)lds; l.stream = stream; l.in_flight = true;
    l.n_streams = 0; l.tables = 0; l.tables_kind = -1; l.tables_born = 0;
    (void)stream_state(stream);
    check_launch(l, fn, args);
    {
        Op op; op.stream = stream; op.type = OP_LAUNCH; op.what = l.kernel; op.launch_seq = l.seq; op.spans = l.spans;
        enqueue(std::move(op));
    }
    float ms = 1.f;
    for (auto& s : g_scripts) if (!s.second.empty() && has(l.kernel, s.first.c_str())) { ms = s.second.front(); s.second.pop_front(); break; }
    g_durations.push_back(ms);
    g_launches.push_back(l);
    if (g_trace) {
        fprintf(g_trace, "{\"seq\": %llu, \"case\": \"%s\", \"kernel\": \"%s\", \"grid\": %u, \"block\": %u, \"lds\": %u, \"n_streams\": %u, \"tables\": \"%s\", \"tables_id\": %llu, \"ms\": %g}\n",
                (unsigned long long)l.seq, l.label.c_str(), l.kernel.c_str(), l.grid, l.block, l.lds, l.n_streams, kind_name(l.tables_kind), (unsigned long long)l.tables_born, ms);
    }
    for (auto& ef : g_effects) if (has(l.kernel, ef.first.c_str())) ef.second(g_launches.back());
    return hipSuccess;
}
