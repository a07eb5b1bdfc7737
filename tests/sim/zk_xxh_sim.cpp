// zk_xxh_sim.cpp -- TEST HARNESS (never shipped, never linked into libzeekstd_amd.so).
// Runs the six XXH64 kernels of the decoder (zeekstd_amd/csrc/zk_xxh64.h, the very source hipcc compiles for gfx950 as part of
// zk_decode.hip) on the CPU, workgroup after workgroup, under the fiber emulator of hip_wg_emu.h, with the launchers' grids and block
// sizes (zk_launch_xxh64 / zk_launch_xxh64_follow: the plans of zk_dec_plan.h).  tests/test_sim_xxh64.py compares what they leave with the
// oracle's XXH64; tests/sim/xxh_san.cpp runs the same under AddressSanitizer + UBSan.
//   Every buffer a kernel sees is a heap allocation of EXACTLY the size the engine gives it: the frames' bytes end where the last frame
// ends, and begin `align` bytes behind a 16-byte boundary (under AddressSanitizer those bytes in front are poisoned too).
//   THE FOLLOWERS run against a SCRIPT in the executor's place: events (step, frame, bytes, xcd, abort) that publish a frame's progress
// word -- and, just before it, the bytes the word announces; every byte not yet announced holds 0xA5.  A wave sees the script from its
// start (the followers are launched beside the executors): before each workgroup the words and the bytes are reset, the events of step 0
// are applied, and the events of step s when the wave polls for the s-th time (hip_wg_emu.h: once per poll of a wave, at its sleep,
// never between a lane's load of a word and its verdict).  The emulated clock advances by `tick` per poll.  A wave that polls more than
// `max_polls` times is cancelled and the run returns 1.
#include "hip_wg_emu.h"
#include "../../zeekstd_amd/csrc/zk_xxh64.h"
#include "../../zeekstd_amd/csrc/zk_dec_plan.h"
#include <memory>
#if defined(__SANITIZE_ADDRESS__)
#include <sanitizer/asan_interface.h>
#define ZKX_ASAN_POISON(p, n) __asan_poison_memory_region((p), (n))
#define ZKX_ASAN_UNPOISON(p, n) __asan_unpoison_memory_region((p), (n))
#else
#define ZKX_ASAN_POISON(p, n) ((void)0)
#define ZKX_ASAN_UNPOISON(p, n) ((void)0)
#endif

template <class T> static std::unique_ptr<T[]> zkx_exact(size_t n) { return std::unique_ptr<T[]>(new T[n ? n : 1]); }
// n bytes that begin `align` (0..15) bytes behind a 16-byte boundary and end where the allocation ends
struct ZkxBytes {
    uint8_t *base, *p;
    ZkxBytes(size_t n, uint32_t a) : base((uint8_t *)malloc(n + a + (n + a == 0))), p(base + a)
    {
        if (!base || ((uintptr_t)base & 15)) abort();       // (malloc's blocks begin on a 16-byte boundary here)
        ZKX_ASAN_POISON(base, a);
    }
    ~ZkxBytes() { ZKX_ASAN_UNPOISON(base, (size_t)(p - base)); free(base); }
    ZkxBytes(const ZkxBytes &) = delete;
};

// out[8]: ZK_XXW, the lean width, the followers' width, ZK_XF_CHUNK, the fed kernel's depth D at four frames, ZK_FOLLOW_PATIENCE,
// ZK_PROG_ABORT's, _VERIFIED's and _MISMATCH's bit numbers packed as a | b << 8 | c << 16, ZK_E_CHECKSUM_WRONG
extern "C" void zk_xxh_sim_consts(uint64_t *out)
{
    out[0] = ZK_XXW; out[1] = ZK_XXL; out[2] = ZK_FOLLOW_W; out[3] = ZK_XF_CHUNK; out[4] = zk_xf_depth(4); out[5] = ZK_FOLLOW_PATIENCE;
    out[6] = (uint64_t)__builtin_ctzll(ZK_PROG_ABORT) | (uint64_t)__builtin_ctzll(ZK_PROG_VERIFIED) << 8 | (uint64_t)__builtin_ctzll(ZK_PROG_MISMATCH) << 16;
    out[7] = ZK_E_CHECKSUM_WRONG;
}
// zk_xxh_plan(count, {xxh = choice}, skip) -> kernel | frames per workgroup << 8; zk_xxh_follow_plan(count) -> follow1 | grid << 8
extern "C" uint32_t zk_xxh_sim_plan(uint32_t count, int choice, int skip)
{
    ZkKernelChoice k; k.xxh = choice;
    const ZkXxhPlan p = zk_xxh_plan(count, k, skip != 0);
    return (uint32_t)p.kernel | p.frames_per_wg << 8;
}
extern "C" uint32_t zk_xxh_sim_follow_plan(uint32_t count)
{
    const ZkXxhFollowPlan p = zk_xxh_follow_plan(count);
    return (uint32_t)p.follow1 | p.grid << 8;
}

static std::unique_ptr<ZkFrameInfo[]> zkx_infos(uint32_t count, const uint32_t *status, const uint32_t *flag, const uint32_t *checksum)
{
    auto infos = zkx_exact<ZkFrameInfo>(count);
    memset(infos.get(), 0xA5, sizeof(ZkFrameInfo) * (count ? count : 1));
    for (uint32_t f = 0; f < count; f++) { infos[f].status = status[f]; infos[f].checksum_flag = flag[f]; infos[f].checksum = checksum[f]; }
    return infos;
}

// One of the passes behind the executor: kernel = ZkXxhKernel (0 zk_k_xxh64, 1 _wide, 2 _lean, 3 _fed<4>), with zk_launch_xxh64's grid.
// bytes[nbytes]: the frames d_off[first] ... d_off[first + count], d_off[first + count + 1] as the caller has it.  status != nullptr: the
// decoder form (infos from status / flag / checksum; status is written back); hashes (in: what the slots hold before, out) and skip may
// be null.  -> 0, -1 for arguments the launcher would not be given.
extern "C" int zk_xxh_sim_pass(int kernel, const uint8_t *bytes, uint64_t nbytes, uint32_t align, const uint64_t *d_off_in, uint32_t first, uint32_t count,
                               uint32_t *status, const uint32_t *flag, const uint32_t *checksum, uint64_t *hashes_io, const uint64_t *skip_in, int descending)
{
    if (count == 0 || align > 15 || d_off_in[first + count] - d_off_in[first] != nbytes) return -1;
    if (skip_in && kernel != ZK_XXH_WIDE && kernel != ZK_XXH_FED4) return -1;
    ZkxBytes data(nbytes, align);
    memcpy(data.p, bytes, nbytes);
    const auto d_off = zkx_exact<uint64_t>((size_t)first + count + 1);
    memcpy(d_off.get(), d_off_in, ((size_t)first + count + 1) * 8);
    std::unique_ptr<ZkFrameInfo[]> infos_h;
    if (status) infos_h = zkx_infos(count, status, flag, checksum);
    std::unique_ptr<uint64_t[]> hashes_h, skip_h;
    if (hashes_io) { hashes_h = zkx_exact<uint64_t>(count); memcpy(hashes_h.get(), hashes_io, (size_t)count * 8); }
    if (skip_in) { skip_h = zkx_exact<uint64_t>(count); memcpy(skip_h.get(), skip_in, (size_t)count * 8); }
    ZkFrameInfo *infos = infos_h.get();
    uint64_t *hashes = hashes_h.get();
    const uint64_t *skip = skip_h.get();
    const uint8_t *dp = data.p;
    const uint64_t *dof = d_off.get();
    emu_set_lane_order(descending != 0);
    g_emu_poll = EmuPoll();
    // zk_launch_xxh64: "grid((count + p.frames_per_wg - 1) / p.frames_per_wg)", dim3(64) -- dim3(128) for zk_k_xxh64_fed<4>
    const uint32_t per = kernel == ZK_XXH_FRAME ? 1 : kernel == ZK_XXH_FED4 ? 4 : 16, grid = (count + per - 1) / per;
    for (uint32_t b = 0; b < grid; b++) switch (kernel) {
        case ZK_XXH_FRAME: emu_run_workgroup(64, b, [&] { zk_k_xxh64(dp, dof, first, count, infos, hashes); }, grid); break;
        case ZK_XXH_WIDE: emu_run_workgroup(64, b, [&] { zk_k_xxh64_wide(dp, dof, first, count, infos, hashes, skip); }, grid); break;
        case ZK_XXH_LEAN: emu_run_workgroup(64, b, [&] { zk_k_xxh64_lean(dp, dof, first, count, infos, hashes); }, grid); break;
        case ZK_XXH_FED4: emu_run_workgroup(128, b, [&] { zk_k_xxh64_fed<4>(dp, dof, first, count, infos, hashes, skip); }, grid); break;
        default: return -1;
    }
    if (status) for (uint32_t f = 0; f < count; f++) status[f] = infos[f].status;
    if (hashes_io) memcpy(hashes_io, hashes, (size_t)count * 8);
    return 0;
}

// the script: at `step` the executor of `frame` publishes `bytes` complete from XCD `xcd` (abort != 0: ZK_PROG_ABORT, as zk_publish(word, 0,
// ZK_PROG_ABORT) does: bytes 0).  Sorted by step; a frame's bytes only grow.
struct ZkxEvent { uint32_t step, frame, bytes, xcd, abort; };

// zk_k_xxh64_follow / _follow1, whichever zk_xxh_follow_plan(count) takes, with its grid; workgroup b runs on XCD wg_xcd[b].
// progress_out[count]: each frame's word as the script leaves it at its end | the bits the waves set.  polls_out[grid]: how often each
// wave polled.  -> 0; 1: a wave polled more than max_polls times and was cancelled; -1: arguments.
extern "C" int zk_xxh_sim_follow(const uint8_t *bytes, uint64_t nbytes, uint32_t align, const uint64_t *d_off_in, uint32_t first, uint32_t count,
                                 const uint32_t *status, const uint32_t *flag, const uint32_t *checksum, const ZkxEvent *ev, uint32_t nev,
                                 const uint32_t *wg_xcd, uint64_t tick, uint64_t max_polls, int descending, uint64_t *progress_out, uint64_t *polls_out)
{
    if (count == 0 || align > 15 || d_off_in[first + count] - d_off_in[first] != nbytes) return -1;
    for (uint32_t e = 0; e < nev; e++) {
        if (ev[e].frame >= count || ev[e].xcd > 7 || (e && ev[e].step < ev[e - 1].step)) return -1;
        if (ev[e].bytes > d_off_in[first + ev[e].frame + 1] - d_off_in[first + ev[e].frame]) return -1;
    }
    ZkxBytes data(nbytes, align);
    const auto d_off = zkx_exact<uint64_t>((size_t)first + count + 1);
    memcpy(d_off.get(), d_off_in, ((size_t)first + count + 1) * 8);
    const auto infos_h = zkx_infos(count, status, flag, checksum);
    const auto progress_h = zkx_exact<uint64_t>(count), bits = zkx_exact<uint64_t>(count), have = zkx_exact<uint64_t>(count);
    const ZkFrameInfo *infos = infos_h.get();
    uint64_t *progress = progress_h.get();
    const uint8_t *dp = data.p;
    const uint64_t *dof = d_off.get();
    memset(bits.get(), 0, (size_t)count * 8);
    const ZkXxhFollowPlan plan = zk_xxh_follow_plan(count);
    uint32_t next = 0;
    // the events whose step has come: first the bytes, then the word
    const auto advance = [&](uint64_t step) {
        for (; next < nev && ev[next].step <= step; next++) {
            const ZkxEvent &e = ev[next];
            const uint64_t at = dof[first + e.frame] - dof[first];
            if (e.bytes > have[e.frame]) { memcpy(data.p + at + have[e.frame], bytes + at + have[e.frame], e.bytes - have[e.frame]); have[e.frame] = e.bytes; }
            progress[e.frame] = (e.abort ? ZK_PROG_ABORT : 0) | (uint64_t)(e.xcd + 1) << 32 | (e.abort ? 0 : e.bytes);
        }
    };
    emu_set_lane_order(descending != 0);
    int rc = 0;
    for (uint32_t b = 0; b < plan.grid && rc == 0; b++) {
        memset(data.p, 0xA5, nbytes);
        memset(progress, 0, (size_t)count * 8);
        memset(have.get(), 0, (size_t)count * 8);
        next = 0;
        g_emu_poll = EmuPoll();
        g_emu_poll.tick = tick; g_emu_poll.max_polls = max_polls; g_emu_poll.xcc = wg_xcd[b];
        g_emu_poll.on_poll = [&] { advance(g_emu_poll.polls); };
        advance(0);
        if (plan.follow1) emu_run_workgroup(64, b, [&] { zk_k_xxh64_follow1(dp, dof, first, count, infos, progress); }, plan.grid);
        else emu_run_workgroup(64, b, [&] { zk_k_xxh64_follow(dp, dof, first, count, infos, progress); }, plan.grid);
        if (emu_cancelled()) rc = 1;
        if (polls_out) polls_out[b] = g_emu_poll.polls;
        for (uint32_t f = 0; f < count; f++) bits[f] |= progress[f] & (ZK_PROG_VERIFIED | ZK_PROG_MISMATCH);
    }
    // the script to its end (what the pass behind the executor finds), and the followers' bits
    advance(~0ull);
    for (uint32_t f = 0; f < count; f++) progress_out[f] = (progress[f] & ~(ZK_PROG_VERIFIED | ZK_PROG_MISMATCH)) | bits[f];
    g_emu_poll = EmuPoll();
    return rc;
}
