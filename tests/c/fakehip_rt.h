// fakehip_rt.h -- TEST HARNESS: the driver's side of tests/c/fakehip_rt.cpp, a recording HIP runtime for the CPU.
// The runtime symbols themselves are the real ones of <hip/hip_runtime_api.h>; this header adds what only a test driver needs:
// the device's capacity, scripted launch times, failure injection, effects, and a look at the ledger and the launch records.
#ifndef DIVANS_TESTS_FAKEHIP_RT_H_
#define DIVANS_TESTS_FAKEHIP_RT_H_
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

namespace fakehip {

enum Kind : int { KIND_BLOCK = 0, KIND_CHUNK = 1, KIND_RESERVED = 2, KIND_HOST = 3 };

struct LedgerEntry {
    uintptr_t base; size_t bytes; int kind; int device; bool alive;
    uint64_t last_launch;      // sequence number of the last launch that referenced it (0: none)
    uint64_t born;             // allocation order
};

// one stretch of a ledger range a queued entry touches: `born` names the range, [lo, hi) the addresses, `write` is false only where
// the argument struct declares the pointer const (or the entry is a copy's source)
struct Span { uint64_t born; uintptr_t lo, hi; bool write; };

struct Launch {
    uint64_t seq;              // 1, 2, ... over the process
    std::string kernel;        // demangled
    std::string label;         // set_case() at the time of the launch
    uint32_t grid, block, lds;
    void* stream;
    bool in_flight;
    uint32_t n_streams;        // of the argument struct, 0 where the kernel has none
    uintptr_t tables; int tables_kind; uint64_t tables_born;     // LitBatch kernels: where the tables lie (Kind), which allocation
    std::vector<uint64_t> refs;                                  // `born` of every ledger entry a pointer of the arguments lies in
    std::vector<uint8_t> args;                                   // the first by-value struct, copied
    std::vector<Span> spans;                                     // what the `order` rule compares: every checked pointer with its extent
};

// what Launch::args holds for the two kernels of the pack pass, which take plain arguments and no struct
struct ScanArgs { const uint32_t* sizes; uint32_t n; uint64_t* offsets; uint64_t* total; int accumulate; };
struct PackArgs { const uint8_t* slots; const uint64_t* src_off; const uint32_t* sizes; uint32_t n; uint8_t* packed; const uint64_t* dst_off; uint64_t cap; uint32_t* status; };

// ---- the device --------------------------------------------------------------------------------------------------------------
void set_capacity(size_t bytes);             // device memory; hipMalloc / hipMemCreate fail beyond it, hipMemGetInfo answers from it
size_t live_bytes();                         // blocks + physical chunks alive
size_t reserved_bytes();                     // address ranges reserved (never handed back)
size_t peak_live_bytes();                    // the most live_bytes() has been since reset_peak(): what was alive AT an allocation, not after a call
void reset_peak();
// What a fresh hipMalloc / hipHostMalloc block and a freshly mapped chunk hold: `byte` (its first 64 MiB; -1, the default: zero pages).
// A result that changes with the byte depends on memory nobody wrote.
void set_fresh_fill(int byte);

// ---- time --------------------------------------------------------------------------------------------------------------------
// The next launches whose kernel name contains `match` take ms[0], ms[1], ... milliseconds (hipEventElapsedTime adds up the launches
// between two events of a stream); every other launch takes 1 ms.
void script_times(const char* match, const std::vector<float>& ms);

// ---- failure injection ---------------------------------------------------------------------------------------------------------
// The injectable calls: hipMalloc, hipMemCreate, hipMemMap, hipMemAddressReserve, hipLaunchKernel (the error comes back through
// hipGetLastError, as a real launch failure does), hipEventRecord, hipEventSynchronize.
void fail_call(const char* function, uint64_t kth, hipError_t e);      // the kth call of `function` from now (1 = the next)
void fail_at(uint64_t index, hipError_t e);                            // the injectable call number `index` counted from now (1 = the next), whichever it is
uint64_t injectable_calls();                                           // how many have been made so far
const char* injected_function();                                       // what the last injected failure hit ("" = none fired)
void clear_failures();

// ---- effects -------------------------------------------------------------------------------------------------------------------
// What a kernel would have written and the host reads back.  Called after the contract checks of a launch whose name contains `match`.
typedef void (*Effect)(const Launch& l);
void set_effect(const char* match, Effect fn);

// ---- records -------------------------------------------------------------------------------------------------------------------
void set_case(const char* label);
void open_trace(const char* path);           // JSON lines, one per launch and one per {"event": ...} the driver adds
void trace_note(const std::string& json_object_body);      // {"note": true, <body>}
const std::vector<Launch>& launches();
std::vector<LedgerEntry> ledger();
enum StreamKind : int { STREAM_NULL = 0, STREAM_BLOCKING = 1, STREAM_NON_BLOCKING = 2 };
int stream_kind(void* stream);               // -1: not a live stream
size_t pending_entries(void* stream);        // queued entries of one stream nothing has completed yet
// `order` allow-list: a ledger range (named by any address inside it) that streams may share without an edge (tests/c/README.md)
void allow_unordered(const void* inside_range, const char* why);
uint64_t stream_syncs();                     // hipStreamSynchronize calls so far
uint64_t count_calls(const char* function);  // calls of one runtime function so far
void check_clean_end();                      // aborts unless the ledger holds no live block, chunk or pinned host buffer
[[noreturn]] void violation(const std::string& kernel, const std::string& field, const std::string& what);

}  // namespace fakehip
#endif
