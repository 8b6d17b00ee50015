// Phase clocks: the one definition behind the timing builds of the hot kernels.  A timing build (-DMML_OP_TIMING=<block>,
// MML_ST_TIMING=<line>, MML_SEL_TIMING=<line>, MML_SP_TIMING=<line>, MML_VX_TIMING=<kind>, MML_SV_TIMING=<problem>) lets ONE watched
// thread of a kernel add up clock64() deltas per phase into its family's slot array; mml_debug_phase_clocks (capi.hip) reads the array
// and tools/phases.py prints the table.  A family is declared in the file whose kernels write it (a __device__ array is per
// translation unit), and a kernel states only what differs between families, its watch condition:
//
//     #ifdef MML_OP_TIMING
//     PHASE_CLOCK_FAMILY(op, 16);          // the slot array, its entry in the reader's list, PhaseClock_op
//     #define OP_WATCH(cond) (cond)
//     #else
//     PHASE_CLOCK_FAMILY_OFF(op);          // PhaseClock_op is the empty clock
//     #define OP_WATCH(cond) false         // (the condition names the flag's value and must not reach the compiler: even as dead
//     #endif                               //  code it changed k_select's register allocation)
//     ...
//     PhaseClock_op clk(OP_WATCH(tid == 64 && blk == MML_OP_TIMING && ...));
//     ...  clk.mark(3);  ...  clk.count(7);
//
// Without the flag the clock is an empty object: no register, no instruction, no __device__ symbol -- the default build's device
// assembly is the same with and without the clocks.  Two clocks in one kernel are two objects; a callee takes one as an argument.
// Not covered: MML_FW_TIMING (fullwindow_dev.hip) sums wall_clock64 spans in the full-window solve's LDS state across launches and
// reports through FwDevOut -- a different instrument with its own read-out.
#pragma once
#include <hip/hip_runtime.h>

// the families a library was built with, for the reader: called once per PHASE_CLOCK_FAMILY before main (capi.hip)
int phase_clock_register(const char* family, const void* symbol, int slots);
constexpr int PHASE_CLOCK_MAX_SLOTS = 64;

template <unsigned long long* SLOTS>
struct PhaseClock {
    static constexpr bool on = true;
    bool watched;             // am I the watched thread
    unsigned long long prev;  // the previous mark
    __device__ __forceinline__ explicit PhaseClock(bool watch) : watched(watch), prev(clock64()) {}
    __device__ __forceinline__ void mark(int id) {  // slot id += cycles since the previous mark
        if (watched) {
            const unsigned long long now = clock64();
            SLOTS[id] += now - prev;
            prev = now;
        }
    }
    __device__ __forceinline__ void count(int id) const {  // slot id += 1
        if (watched) SLOTS[id] += 1;
    }
    __device__ __forceinline__ void stamp(int id) const {  // slot id = the clock (k_select: a line's last pass through each mark)
        if (watched) SLOTS[id] = clock64();
    }
};
template <>
struct PhaseClock<nullptr> {
    static constexpr bool on = false;
    __device__ __forceinline__ explicit PhaseClock(bool) {}
    __device__ __forceinline__ void mark(int) const {}
    __device__ __forceinline__ void count(int) const {}
    __device__ __forceinline__ void stamp(int) const {}
};

#define PHASE_CLOCK_FAMILY(fam, n)                                                                                         \
    static_assert((n) <= PHASE_CLOCK_MAX_SLOTS, "phase clock family " #fam ": more slots than the reader clears");          \
    __device__ unsigned long long g_##fam##_dbg[n];                                                                        \
    static const int g_##fam##_dbg_listed = phase_clock_register(#fam, reinterpret_cast<const void*>(g_##fam##_dbg), n); \
    using PhaseClock_##fam = PhaseClock<g_##fam##_dbg>
#define PHASE_CLOCK_FAMILY_OFF(fam) using PhaseClock_##fam = PhaseClock<nullptr>
