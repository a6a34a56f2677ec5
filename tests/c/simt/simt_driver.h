// TEST HARNESS: what a driver program asks of the lane-lockstep stand-in (tests/c/simt/simt.cpp) apart from the device side of
// hip/hip_runtime.h: the poison byte and a look at what ran.  Included by simt.cpp too, so the two cannot drift apart.
#ifndef DIVANS_TESTS_SIMT_DRIVER_H_
#define DIVANS_TESTS_SIMT_DRIVER_H_
#include <stdint.h>

#include <string>
#include <utility>
#include <vector>

namespace simt {
void set_poison(int byte);                                        // what fresh LDS holds (default 0xA7)
std::vector<std::pair<std::string, uint64_t>> instances();        // (instance, launches so far), sorted
uint64_t launches_of(const char* instance);                       // instances are spelt as a profiler spells them: "divans_hip::lit_decode2_kernel_any<-1, true, false, false, 17>"
uint32_t last_grid(const char* instance);                         // workgroups of its last launch (0: never launched)
void print_instances();                                           // one "SIMT RAN <instance>  (<launches> launches)" line each
}  // namespace simt
#endif
