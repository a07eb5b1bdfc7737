// hip_wg_emu.h -- TEST HARNESS (never shipped): runs ONE workgroup of a HIP kernel on the CPU, a ucontext fiber per lane.
// The kernel source is compiled unchanged by g++; this header supplies what the device compiler would:
//   __shared__             -> static (one workgroup at a time)
//   __syncthreads / LDS barrier -> every live lane of the workgroup parks until all arrived
//   wave collectives (__ballot, readlane, ds_bpermute, update_dpp row_shr:1, wave_barrier) -> the 64 lanes of a wave
//                             deposit their value and park until the wave is complete; they must be called by all 64
//                             lanes (wave-uniform control flow), as the kernels under test do
//   __shfl / __shfl_xor (32- and 64-bit), __any -> collectives like __ballot; __builtin_amdgcn_alignbit, uint4 / make_uint4
//   atomicCAS / atomicMin / atomicMax / atomicAdd / atomicOr -> plain (fibers are cooperative)
//   zk_xxh64.h's hooks (ZKX_XCC_ID, ZKX_CLOCK, ZKX_SLEEP, ZKX_ACQUIRE, ZKX_PROG_LOAD) -> a scripted neighbour: see POLLING below
//   gridDim, blockIdx.x / .y -> what emu_run_workgroup was told (defaults: a grid of one workgroup)
// The scheduler visits the lanes in ascending order, or -- emu_set_lane_order(true) -- in descending order: a kernel whose result does
// not depend on which lane reaches an atomic first gives the same output under both.
// Lanes of a wave do NOT run in lock step here: code that relies on the in-order LDS pipeline of one wave needs a
// __builtin_amdgcn_wave_barrier() (a scheduling fence on the device, a wave meeting point here).
#pragma once
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <ucontext.h>
#include <functional>
#include <vector>

struct EmuDim { uint32_t x, y, z; };
struct EmuWave { uint32_t vals[64], res[64]; uint32_t count; uint64_t gen; };
struct EmuLane { ucontext_t ctx; uint32_t tid; bool done; };
struct EmuWG {
    ucontext_t sched;
    std::vector<EmuLane> lanes;
    std::vector<EmuWave> waves;
    std::vector<char> stacks;
    uint32_t nthreads = 0, cur = 0, block = 0, live = 0;
    uint32_t block_y = 0, grid_x = 1, grid_y = 1;
    bool descending = false;
    uint32_t bar_count = 0; uint64_t bar_gen = 0;
    std::function<void()> body;
};
static EmuWG g_emu;

static inline void emu_yield() { swapcontext(&g_emu.lanes[g_emu.cur].ctx, &g_emu.sched); }
static inline EmuDim emu_tidx() { return EmuDim{g_emu.lanes[g_emu.cur].tid, 0, 0}; }
static inline EmuDim emu_bidx() { return EmuDim{g_emu.block, g_emu.block_y, 0}; }
static inline EmuDim emu_gdim() { return EmuDim{g_emu.grid_x, g_emu.grid_y, 1}; }
static inline void emu_set_lane_order(bool descending) { g_emu.descending = descending; }

static inline void emu_barrier()
{
    EmuWG &g = g_emu;
    const uint64_t gen = g.bar_gen;
    if (++g.bar_count == g.live) { g.bar_count = 0; g.bar_gen++; return; }
    while (g.bar_gen == gen) emu_yield();
}
// every lane of the wave deposits v; returns the 64 deposited values
static inline const uint32_t *emu_collect(uint32_t v)
{
    EmuWG &g = g_emu;
    const uint32_t tid = g.lanes[g.cur].tid;
    EmuWave &w = g.waves[tid >> 6];
    w.vals[tid & 63] = v;
    const uint64_t gen = w.gen;
    if (++w.count == 64) { w.count = 0; memcpy(w.res, w.vals, sizeof w.res); w.gen++; }
    else while (w.gen == gen) emu_yield();
    return w.res;
}
static inline uint64_t emu_ballot(bool p)
{
    const uint32_t *r = emu_collect(p ? 1u : 0u);
    uint64_t m = 0;
    for (int i = 0; i < 64; i++) m |= (uint64_t)(r[i] & 1) << i;
    return m;
}
static inline int emu_readlane(int v, int l) { return (int)emu_collect((uint32_t)v)[l & 63]; }
static inline int emu_bpermute(int addr, int v)
{
    const uint32_t mine = ((uint32_t)addr >> 2) & 63;        // captured before parking: res[] is shared
    return (int)emu_collect((uint32_t)v)[mine];
}
static inline int emu_dpp(int old, int src, int ctrl)
{
    const uint32_t lane = g_emu.lanes[g_emu.cur].tid & 63;
    const uint32_t *r = emu_collect((uint32_t)src);
    if (ctrl >= 0x111 && ctrl <= 0x11F) {                    // row_shr:n -- lane i of a row of 16 reads lane i - n of the same row
        const uint32_t n = (uint32_t)ctrl - 0x110;
        return (lane & 15) >= n ? (int)r[lane - n] : old;
    }
    if (ctrl >= 0x101 && ctrl <= 0x10F) {                    // row_shl:n
        const uint32_t n = (uint32_t)ctrl - 0x100;
        return (lane & 15) + n < 16 ? (int)r[lane + n] : old;
    }
    abort();
}
static inline void emu_wave_sync() { (void)emu_collect(0); }
static inline uint32_t emu_alignbyte(uint32_t hi, uint32_t lo, uint32_t s) { return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8 * (s & 3))); }
static inline uint32_t emu_atomic_cas(uint32_t *p, uint32_t cmp, uint32_t val) { const uint32_t old = *p; if (old == cmp) *p = val; return old; }

static inline uint32_t emu_atomic_min(uint32_t *p, uint32_t v) { const uint32_t old = *p; if (v < old) *p = v; return old; }
static inline uint32_t emu_atomic_max(uint32_t *p, uint32_t v) { const uint32_t old = *p; if (v > old) *p = v; return old; }
static inline uint32_t emu_atomic_add(uint32_t *p, uint32_t v) { const uint32_t old = *p; *p = old + v; return old; }
template <typename T> static inline T emu_atomic_or(T *p, T v) { const T old = *p; *p = old | v; return old; }
// __shfl / __shfl_xor (width 64) for 32- and 64-bit values, __any: collectives like __ballot
static inline uint32_t emu_shfl32(uint32_t v, uint32_t src) { return emu_collect(v)[src & 63]; }            // (src is read before the lane parks)
static inline uint32_t emu_shfl(uint32_t v, int src, int) { return emu_shfl32(v, (uint32_t)src); }
static inline int emu_shfl(int v, int src, int) { return (int)emu_shfl32((uint32_t)v, (uint32_t)src); }
static inline uint64_t emu_shfl(uint64_t v, int src, int)
{
    const uint32_t lo = emu_shfl32((uint32_t)v, (uint32_t)src), hi = emu_shfl32((uint32_t)(v >> 32), (uint32_t)src);
    return ((uint64_t)hi << 32) | lo;
}
template <typename T> static inline T emu_shfl_xor(T v, int mask, int w) { return emu_shfl(v, (int)((g_emu.lanes[g_emu.cur].tid & 63) ^ (uint32_t)mask), w); }
static inline bool emu_any(bool p) { return emu_ballot(p) != 0; }
static inline uint32_t emu_alignbit(uint32_t hi, uint32_t lo, uint32_t s) { return (uint32_t)((((uint64_t)hi << 32) | lo) >> (s & 31)); }
struct uint4 { uint32_t x, y, z, w; };
static inline uint4 make_uint4(uint32_t x, uint32_t y, uint32_t z, uint32_t w) { return uint4{x, y, z, w}; }

// POLLING (zk_xxh64.h's hooks: a kernel that follows words another kernel writes).  Nothing else runs while a workgroup is emulated, so
// the other kernel is a script: `on_poll` is called ONCE per poll of a wave, at the kernel's sleep, when all 64 lanes have arrived and
// none is between the load of a word and the verdict on it -- there, and nowhere else, progress words, the bytes they announce and the
// clock change.  A verdict that is wave-uniform on the device (readfirstlane, zk_uni: identities here) is then uniform here too, whatever
// the lane order.  `max_polls` bounds a run: a kernel that polls more often than its patience allows is cancelled -- the lanes are
// abandoned where they are, emu_run_workgroup returns and emu_cancelled() says so -- instead of spinning for ever.  (Abandoned: the lane
// that trips the bound yields for ever and no fiber's stack is unwound, so nothing a kernel holds may need a destructor -- true of the
// kernels here, which hold plain values.)  emu_poll counts arrivals in the wave's `count` / `gen`, the words emu_collect uses: like
// every collective it must be reached by all 64 lanes, with no lane parked in another collective meanwhile -- wave-uniform control flow
// between a collective and a sleep, which is what the device asks of these loops too.
struct EmuPoll { std::function<void()> on_poll; uint64_t clock = 0, tick = 1, polls = 0, max_polls = ~0ull; uint32_t xcc = 0; };
static EmuPoll g_emu_poll;
static bool g_emu_cancel = false;
static inline bool emu_cancelled() { return g_emu_cancel; }
static inline void emu_poll()
{
    EmuWG &g = g_emu;
    EmuWave &w = g.waves[g.lanes[g.cur].tid >> 6];
    const uint64_t gen = w.gen;
    if (++w.count < 64) { while (w.gen == gen) emu_yield(); return; }
    w.count = 0;
    g_emu_poll.clock += g_emu_poll.tick;
    if (++g_emu_poll.polls > g_emu_poll.max_polls) { g_emu_cancel = true; for (;;) emu_yield(); }
    if (g_emu_poll.on_poll) g_emu_poll.on_poll();
    w.gen++;
}

static void emu_entry()
{
    g_emu.body();
    EmuWG &g = g_emu;
    g.lanes[g.cur].done = true;
    g.live--;
    swapcontext(&g.lanes[g.cur].ctx, &g.sched);
}

// run `body` (the kernel call) as workgroup (`block`, `block_y`) of `nthreads` lanes in a grid of grid_x x grid_y workgroups
static void emu_run_workgroup(uint32_t nthreads, uint32_t block, std::function<void()> body, uint32_t grid_x = 1, uint32_t block_y = 0, uint32_t grid_y = 1)
{
    EmuWG &g = g_emu;
    constexpr size_t STACK = 128 << 10;
    g.nthreads = nthreads; g.block = block; g.live = nthreads; g.body = body;
    g.block_y = block_y; g.grid_x = grid_x; g.grid_y = grid_y;
    g.bar_count = 0;
    g.lanes.assign(nthreads, EmuLane());
    g.waves.assign((nthreads + 63) / 64, EmuWave());
    if (g.stacks.size() < STACK * nthreads) g.stacks.resize(STACK * nthreads);
    for (uint32_t t = 0; t < nthreads; t++) {
        EmuLane &l = g.lanes[t];
        l.tid = t; l.done = false;
        getcontext(&l.ctx);
        l.ctx.uc_stack.ss_sp = g.stacks.data() + STACK * t;
        l.ctx.uc_stack.ss_size = STACK;
        l.ctx.uc_link = &g.sched;
        makecontext(&l.ctx, emu_entry, 0);
    }
    g_emu_cancel = false;
    while (g.live && !g_emu_cancel) {
        for (uint32_t i = 0; i < nthreads && !g_emu_cancel; i++) {
            const uint32_t t = g.descending ? nthreads - 1 - i : i;
            if (g.lanes[t].done) continue;
            g.cur = t;
            swapcontext(&g.sched, &g.lanes[t].ctx);
        }
    }
}

#define __global__
#define __device__
#define __forceinline__ inline
#define __shared__ static
#define __launch_bounds__(...)
#define threadIdx (emu_tidx())
#define blockIdx (emu_bidx())
#define gridDim (emu_gdim())
#define __syncthreads() emu_barrier()
#define ZKE_LDS_BARRIER() emu_barrier()
#define __ballot(p) emu_ballot(p)
#define __builtin_amdgcn_readlane(v, l) emu_readlane((v), (l))
#define __builtin_amdgcn_ds_bpermute(a, v) emu_bpermute((a), (v))
#define __builtin_amdgcn_update_dpp(old, src, ctrl, rm, bm, bc) emu_dpp((old), (src), (ctrl))
#define __builtin_amdgcn_alignbyte(hi, lo, s) emu_alignbyte((hi), (lo), (s))
#define __builtin_amdgcn_wave_barrier() emu_wave_sync()
#define ZKE_WAVE_SYNC() emu_wave_sync()
#define __builtin_amdgcn_readfirstlane(v) (v)          /* only used on values that are uniform across the wave */
#define atomicCAS(p, c, v) emu_atomic_cas((p), (c), (v))
#define atomicMin(p, v) emu_atomic_min((p), (v))
#define atomicMax(p, v) emu_atomic_max((p), (v))
#define atomicAdd(p, v) emu_atomic_add((p), (v))
#define atomicOr(p, v) emu_atomic_or((p), (__typeof__(*(p)))(v))
#define __shfl(v, l, w) emu_shfl((v), (int)(l), (w))
#define __shfl_xor(v, m, w) emu_shfl_xor((v), (m), (w))
#define __any(p) emu_any(p)
#define __popcll(x) __builtin_popcountll(x)
#define __builtin_amdgcn_alignbit(hi, lo, s) emu_alignbit((hi), (lo), (s))
#define ZKX_XCC_ID() (g_emu_poll.xcc)
#define ZKX_CLOCK() (g_emu_poll.clock)
#define ZKX_SLEEP(n) emu_poll()
#define ZKX_ACQUIRE() ((void)0)
#define ZKX_PROG_LOAD(p) (*(const volatile uint64_t *)(p))
#define __ffs(x) __builtin_ffs(x)
#define ZKE_FFBL(x) ((x) ? (uint32_t)__builtin_ctz(x) : 0xFFFFFFFFu)          /* v_ffbl_b32 */
#define ZKE_FFBH(x) ((x) ? (uint32_t)__builtin_clz(x) : 0xFFFFFFFFu)          /* v_ffbh_u32 */
#define ZKE_WALK(taken, f, nx) do { taken |= 1ull << f; f = (uint32_t)emu_readlane((int)(nx), (int)f); } while (f < 64)     /* zk_enc_match2.h: the walk's inner loop */
#define ZKE_KEEP(x) do { } while (0)
