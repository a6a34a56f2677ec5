// TEST HARNESS: the lane scheduler behind tests/c/simt/hip/hip_runtime.h.  One fiber (ucontext) per lane of the workgroup that is
// running, one lane at a time, deterministic: a lane runs until it parks at a cross-lane operation or a barrier (or returns), then the
// next runnable lane of its wave runs; when no lane of the wave can run, the lanes parked at the call site that comes first in the
// code are the exec mask: their operation is carried out with wave64 semantics and they go on.  A barrier opens when every live lane of the workgroup waits
// at it.  Built with -fsanitize=address,undefined like the kernels it runs (the fiber switches are announced to AddressSanitizer).
#include <hip/hip_runtime.h>

#include "simt_driver.h"

#include <cxxabi.h>
#include <dlfcn.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <sys/mman.h>
#include <ucontext.h>

#include <algorithm>
#include <map>
#include <string>
#include <vector>

#if defined(__has_feature)
#if __has_feature(address_sanitizer)
#define SIMT_ASAN 1
#endif
#endif
#if defined(__SANITIZE_ADDRESS__) && !defined(SIMT_ASAN)
#define SIMT_ASAN 1
#endif
#ifdef SIMT_ASAN
#include <sanitizer/common_interface_defs.h>
#endif

namespace simt {
namespace {

constexpr size_t kStackBytes = (size_t)256 << 10;
constexpr uint32_t kWave = 64, kMaxLanes = 1024;
constexpr uint32_t kMaxLds = 160u << 10;      // of a CU

enum State : uint8_t { RUNNABLE, PARKED, BARRIER, DEAD };
enum OpKind : uint8_t { OP_DPP, OP_BPERMUTE, OP_READFIRSTLANE, OP_BALLOT, OP_SHFL_XOR, OP_LDS_READ, OP_LDS_WRITE, OP_SYNC };

struct Fiber {
    ucontext_t uc;
    void* fake_stack = nullptr;
    const void* bottom = nullptr; size_t size = 0;
};
struct Lane : Fiber {
    int a = 0, b = 0, ctrl = 0; bool flag = false;      // operands
    unsigned long long result = 0;
    LaneIds ids;
    uint32_t index = 0;
};

struct Group {
    std::vector<Lane> lanes;
    // what the scheduler scans, apart from the fibers (a ucontext_t is a kilobyte): state, operation and call site of every lane
    State state[kMaxLanes]; OpKind op[kMaxLanes]; const void* site[kMaxLanes];
    uint32_t n = 0, live = 0;
    Lane* cur = nullptr;
    Fiber main;
    const std::function<void()>* body = nullptr;
    uint8_t* lds = nullptr; uint32_t lds_bytes = 0;
    std::map<std::pair<std::string, int>, uint8_t*> statics;
    std::string kernel;
    uint32_t block = 0;
    uint8_t* stacks = nullptr;
    bool from_main = false;
};
Group g;
int g_poison = 0xA7;
std::map<std::string, uint64_t> g_ran;
std::map<std::string, uint32_t> g_grid;

void switch_to(Fiber* from, Fiber* to, bool from_ends) {
#ifdef SIMT_ASAN
    __sanitizer_start_switch_fiber(from_ends ? nullptr : &from->fake_stack, to->bottom, to->size);
#endif
    swapcontext(&from->uc, &to->uc);
#ifdef SIMT_ASAN
    __sanitizer_finish_switch_fiber(from->fake_stack, nullptr, nullptr);
#endif
}

[[noreturn]] void report_stuck(const char* why) {
    fprintf(stderr, "SIMT FINDING: kernel %s, workgroup %u: %s\n", g.kernel.c_str(), g.block, why);
    for (uint32_t i = 0; i < g.n; ++i) {
        if (g.state[i] == PARKED || g.state[i] == BARRIER) fprintf(stderr, "  lane %u parked at %p (%s)\n", i, g.site[i], g.state[i] == BARRIER ? "barrier" : "cross-lane operation");
    }
    abort();
}

// the lane `ctrl` names as lane i's source inside its row of 16, or -1 (the lane reads `old` / 0)
int dpp_source(int ctrl, int i) {
    if (ctrl >= 0 && ctrl <= 0xff) return (i & ~3) | ((ctrl >> (2 * (i & 3))) & 3);        // quad_perm
    if (ctrl >= 0x101 && ctrl <= 0x10f) { const int s = i + (ctrl - 0x100); return s < 16 ? s : -1; }     // row_shl
    if (ctrl >= 0x111 && ctrl <= 0x11f) { const int s = i - (ctrl - 0x110); return s >= 0 ? s : -1; }     // row_shr
    if (ctrl >= 0x121 && ctrl <= 0x12f) return (i - (ctrl - 0x120)) & 15;                  // row_ror
    if (ctrl == 0x140) return 15 - i;                                                     // row_mirror
    if (ctrl == 0x141) return (i & 8) | (7 - (i & 7));                                    // row_half_mirror
    if (ctrl >= 0x150 && ctrl <= 0x15f) return ctrl - 0x150;                              // row_newbcast
    finding("DPP control 0x%x is not modelled", ctrl);
}

// carries out one call site's operation for the lanes of the wave that are parked at it; false if none is parked at one
bool resolve_wave(uint32_t w) {
    const uint32_t lo = w * kWave, hi = std::min(lo + kWave, g.n);
    // Of the call sites lanes wait at, the one that comes first in the code goes on alone (the lowest address: the kernel is one
    // function, every helper inlined): lanes that took a longer path catch up with the ones that wait further down before those
    // go on, as a wave's reconvergence has it -- a lane never passes a fence while another has stores in front of it still to do.
    const void* lowest = nullptr;
    for (uint32_t i = lo; i < hi; ++i) if (g.state[i] == PARKED && (!lowest || g.site[i] < lowest)) lowest = g.site[i];
    if (!lowest) return false;
    bool any = false;
    for (uint32_t first = lo; first < hi && !any; ++first) {
        if (g.state[first] != PARKED || g.site[first] != lowest) continue;
        const Lane& f = g.lanes[first];
        const OpKind fop = g.op[first];
        any = true;
        unsigned long long mask = 0;
        for (uint32_t i = first; i < hi; ++i) if (g.state[i] == PARKED && g.site[i] == lowest && g.op[i] == fop) mask |= 1ull << (i - lo);
        auto in = [&](int lane) { return lane >= 0 && ((mask >> lane) & 1ull) != 0; };
        unsigned long long ballot_bits = 0;
        if (fop == OP_BALLOT) for (uint32_t i = first; i < hi; ++i) if (in((int)(i - lo)) && g.lanes[i].flag) ballot_bits |= 1ull << (i - lo);
        unsigned long long results[kWave];
        for (uint32_t i = first; i < hi; ++i) {
            const int k = (int)(i - lo);
            if (!in(k)) continue;
            const Lane& l = g.lanes[i];
            unsigned long long r = 0;
            switch (fop) {
            case OP_DPP: {
                const int s = dpp_source(l.ctrl, k & 15);
                const int src = s < 0 ? -1 : (k & ~15) | s;
                r = in(src) ? (unsigned)g.lanes[lo + src].b : (l.flag ? 0u : (unsigned)l.a);
                break;
            }
            case OP_BPERMUTE: { const int src = (l.a >> 2) & 63; r = in(src) ? (unsigned)g.lanes[lo + src].b : 0u; break; }
            case OP_READFIRSTLANE: r = (unsigned)f.a; break;
            case OP_BALLOT: r = ballot_bits; break;
            case OP_LDS_READ: memcpy(&r, g.lds + (uint32_t)l.a, (size_t)l.ctrl); break;          // (bounds: checked by the lane before it parked)
            case OP_LDS_WRITE: case OP_SYNC: break;
            case OP_SHFL_XOR: { const int src = k ^ (l.b & 63); r = in(src) ? (unsigned)g.lanes[lo + src].a : (unsigned)l.a; break; }
            }
            results[k] = r;
        }
        for (uint32_t i = first; i < hi; ++i) {
            if (!in((int)(i - lo))) continue;
            Lane& l = g.lanes[i];
            if (fop == OP_LDS_WRITE) memcpy(g.lds + (uint32_t)l.a, &l.b, (size_t)l.ctrl);      // in lane order, behind every read of the group before
            l.result = results[i - lo]; g.state[i] = RUNNABLE;
        }
    }
    return any;
}

// the lane to run after `from` has parked or ended; nullptr when every lane has returned
Lane* pick_next(const Lane* from) {
    const uint32_t waves = (g.n + kWave - 1) / kWave, w0 = from->index / kWave;
    for (;;) {
        if (g.live == 0) return nullptr;
        for (uint32_t dw = 0; dw < waves; ++dw) {
            const uint32_t w = (w0 + dw) % waves, lo = w * kWave, cnt = std::min(kWave, g.n - lo);
            const uint32_t start = dw == 0 ? (from->index - lo + 1) % cnt : 0;
            for (int pass = 0; pass < 2; ++pass) {
                for (uint32_t k = 0; k < cnt; ++k) { const uint32_t i = lo + (start + k) % cnt; if (g.state[i] == RUNNABLE) return &g.lanes[i]; }
                if (pass == 0 && !resolve_wave(w)) break;
            }
        }
        // no lane of any wave can run and none waits at a cross-lane operation: every live lane waits at a barrier
        const void* site = nullptr;
        for (uint32_t i = 0; i < g.n; ++i) {
            if (g.state[i] != BARRIER) continue;
            if (site && g.site[i] != site) report_stuck("live lanes wait at different barriers and no lane can run");
            site = g.site[i];
        }
        if (!site) report_stuck("no lane can run");
        for (uint32_t i = 0; i < g.n; ++i) if (g.state[i] == BARRIER) g.state[i] = RUNNABLE;
    }
}

void lane_entry() {
#ifdef SIMT_ASAN
    {
        const void* bottom = nullptr; size_t size = 0;
        __sanitizer_finish_switch_fiber(nullptr, &bottom, &size);
        if (g.from_main) { g.main.bottom = bottom; g.main.size = size; }      // the first lane is entered from the launching thread's stack
    }
    g.from_main = false;
#endif
    (*g.body)();
    Lane* self = g.cur;
    g.state[self->index] = DEAD;
    --g.live;
    Lane* next = pick_next(self);
    g.cur = next;
    switch_to(self, next ? static_cast<Fiber*>(next) : &g.main, true);
    abort();
}

unsigned long long park(OpKind op, const void* site, int a, int b, int ctrl, bool flag) {
    Lane* self = g.cur;
    if (!self) { fprintf(stderr, "simt: a cross-lane operation outside a kernel\n"); abort(); }
    self->a = a; self->b = b; self->ctrl = ctrl; self->flag = flag;
    g.op[self->index] = op; g.site[self->index] = site; g.state[self->index] = PARKED;
    Lane* next = pick_next(self);
    if (next != self) { g.cur = next; switch_to(self, next, false); }
    return self->result;
}

std::string kernel_name(const void* fn) {
    Dl_info info;
    if (dladdr(fn, &info) && info.dli_sname) {
        int status = 0;
        char* d = abi::__cxa_demangle(info.dli_sname, nullptr, nullptr, &status);
        std::string s = d && status == 0 ? d : info.dli_sname;
        free(d);
        if (s.compare(0, 5, "void ") == 0) s = s.substr(5);
        const size_t args = s.rfind('(');       // the parameter list
        return args == std::string::npos ? s : s.substr(0, args);
    }
    char buf[32]; snprintf(buf, sizeof buf, "kernel@%p", fn);
    return buf;
}

}  // namespace

const LaneIds& ids() { return g.cur->ids; }

void finding(const char* fmt, ...) {
    fprintf(stderr, "SIMT FINDING: kernel %s, workgroup %u, lane %u: ", g.kernel.c_str(), g.block, g.cur ? g.cur->index : 0u);
    va_list ap; va_start(ap, fmt); vfprintf(stderr, fmt, ap); va_end(ap);
    fputc('\n', stderr);
    abort();
}

uint8_t* dynamic_lds() { return g.lds; }
uint8_t* static_lds(const char* file, int line, size_t bytes) {
    uint8_t*& p = g.statics[{file, line}];
    if (!p) { p = (uint8_t*)malloc(bytes ? bytes : 1); memset(p, g_poison, bytes); }
    return p;
}
uint32_t lds_addr(const void* p) {
    const uint8_t* q = (const uint8_t*)p;
    if (q < g.lds || q > g.lds + g.lds_bytes) finding("LDS address taken of %p, which does not point into the workgroup's %u bytes of dynamic LDS", p, g.lds_bytes);
    return (uint32_t)(q - g.lds);
}
uint8_t* lds_at(uint32_t addr, uint32_t bytes) {
    if ((uint64_t)addr + bytes > g.lds_bytes) finding("LDS access of %u bytes at address %u (0x%x): the workgroup's LDS has %u bytes", bytes, addr, addr, g.lds_bytes);
    return g.lds + addr;
}
uint8_t* buffer_at(const BufferRsrc& r, uint32_t off, uint32_t bytes, const char* what) {
    if ((uint64_t)off + bytes > r.num_records) finding("buffer %s of %u bytes at offset %u (0x%x) of a resource with num_records %u (base %p)", what, bytes, off, off, r.num_records, (void*)r.base);
    return r.base + off;
}

int dpp(int old, int src, int ctrl, bool bound_ctrl) { return (int)park(OP_DPP, __builtin_return_address(0), old, src, ctrl, bound_ctrl); }
int bpermute(int byte_addr, int v) { return (int)park(OP_BPERMUTE, __builtin_return_address(0), byte_addr, v, 0, false); }
int readfirstlane(int v) { return (int)park(OP_READFIRSTLANE, __builtin_return_address(0), v, 0, 0, false); }
unsigned long long ballot(bool pred) { return park(OP_BALLOT, __builtin_return_address(0), 0, 0, 0, pred); }
uint32_t lds_read8(uint32_t a) { lds_at(a, 1); return (uint32_t)park(OP_LDS_READ, __builtin_return_address(0), (int)a, 0, 1, false); }
uint32_t lds_read16(uint32_t a) { lds_at(a, 2); return (uint32_t)park(OP_LDS_READ, __builtin_return_address(0), (int)a, 0, 2, false); }
uint32_t lds_read32(uint32_t a) { lds_at(a, 4); return (uint32_t)park(OP_LDS_READ, __builtin_return_address(0), (int)a, 0, 4, false); }
void lds_write16(uint32_t a, uint32_t v) { lds_at(a, 2); park(OP_LDS_WRITE, __builtin_return_address(0), (int)a, (int)v, 2, false); }
void lds_write32(uint32_t a, uint32_t v) { lds_at(a, 4); park(OP_LDS_WRITE, __builtin_return_address(0), (int)a, (int)v, 4, false); }
void wave_sync() { park(OP_SYNC, __builtin_return_address(0), 0, 0, 0, false); }
int shfl_xor(int v, int lane_mask) { return (int)park(OP_SHFL_XOR, __builtin_return_address(0), v, lane_mask, 0, false); }
void syncthreads() {
    Lane* self = g.cur;
    g.site[self->index] = __builtin_return_address(0);
    g.state[self->index] = BARRIER;
    Lane* next = pick_next(self);
    if (next != self) { g.cur = next; switch_to(self, next, false); }
}

void set_poison(int byte) { g_poison = byte & 0xff; }

std::vector<std::pair<std::string, uint64_t>> instances() { return std::vector<std::pair<std::string, uint64_t>>(g_ran.begin(), g_ran.end()); }
uint32_t last_grid(const char* instance) { const auto it = g_grid.find(instance); return it == g_grid.end() ? 0 : it->second; }
uint64_t launches_of(const char* instance) { const auto it = g_ran.find(instance); return it == g_ran.end() ? 0 : it->second; }

void print_instances() {
    for (const auto& kv : g_ran) printf("SIMT RAN %s  (%llu launches)\n", kv.first.c_str(), (unsigned long long)kv.second);
}

hipError_t launch(const void* kernel, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t, const std::function<void()>& body) {
    if (g.cur) { fprintf(stderr, "simt: a launch from inside a kernel\n"); abort(); }
    if (grid.x == 0 || grid.y != 1 || grid.z != 1 || block.x == 0 || block.x > kMaxLanes || block.y != 1 || block.z != 1) { fprintf(stderr, "simt: launch shape %u x %u is not modelled\n", grid.x, block.x); abort(); }
    g.kernel = kernel_name(kernel);
    if (lds_bytes > kMaxLds) { g.block = 0; finding("launch with %zu bytes of dynamic LDS: a CU has %u", lds_bytes, kMaxLds); }
    ++g_ran[g.kernel];
    g_grid[g.kernel] = grid.x;
    if (!g.stacks) {
        g.stacks = (uint8_t*)mmap(nullptr, kStackBytes * kMaxLanes, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
        if (g.stacks == (uint8_t*)MAP_FAILED) { perror("simt: mmap of the lane stacks"); abort(); }
        g.lanes.resize(kMaxLanes);
    }
    g.body = &body;
    g.n = block.x;
    for (uint32_t b = 0; b < grid.x; ++b) {
        g.block = b;
        g.lds_bytes = (uint32_t)lds_bytes;
        g.lds = (uint8_t*)malloc(lds_bytes ? lds_bytes : 1);
        memset(g.lds, g_poison, lds_bytes);
        for (uint32_t i = 0; i < g.n; ++i) {
            Lane& l = g.lanes[i];
            g.state[i] = RUNNABLE; l.index = i; l.fake_stack = nullptr;
            l.ids.thread = {i, 0, 0}; l.ids.block = {b, 0, 0}; l.ids.block_dim = {block.x, 1, 1}; l.ids.grid_dim = {grid.x, 1, 1};
            getcontext(&l.uc);
            l.bottom = g.stacks + kStackBytes * i; l.size = kStackBytes;
            l.uc.uc_stack.ss_sp = (void*)l.bottom; l.uc.uc_stack.ss_size = kStackBytes; l.uc.uc_link = nullptr;
            makecontext(&l.uc, lane_entry, 0);
        }
        g.live = g.n;
        g.cur = &g.lanes[0];
        g.from_main = true;
        switch_to(&g.main, g.cur, false);
        g.cur = nullptr;
        free(g.lds); g.lds = nullptr;
        for (auto& kv : g.statics) free(kv.second);
        g.statics.clear();
    }
    g.body = nullptr;
    return hipSuccess;
}

}  // namespace simt
