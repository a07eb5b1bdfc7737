// zk_enc_match_emu.h -- TEST HARNESS: what zk_enc_sim.cpp and zk_enc_plan_list_sim.cpp share -- the match launcher on the CPU and the copy
// of the blocks' outputs.
#pragma once
#include "hip_wg_emu.h"
#include "../../zeekstd_amd/csrc/zk_enc_match.h"
#include "../../zeekstd_amd/csrc/zk_enc_match2.h"
#include "../../zeekstd_amd/csrc/zk_enc_sched.h"

// zk_launch_enc_match under the emulator: the instance zk_enc_match_kernel names, a workgroup per segment
static void zk_emu_enc_match(const uint8_t *src, const ZkEncFrame *segs, uint32_t nsegs, ZkEncBlock *blocks, uint64_t *seqs, uint8_t *lits, int level, const ZkEncLdm &ldm)
{
    const ZkEncMatchKernel which = zk_enc_match_kernel(level, ldm.table != nullptr, ldm.dense != nullptr);
    auto run = [&]() {
        switch (which) {
#define ZK_EMU_GO(name, kernel, takes_ldm) case name: kernel(src, segs, blocks, seqs, lits ZK_ENC_MATCH_LDM_##takes_ldm(ldm)); break;
        ZK_ENC_MATCH_KERNELS(ZK_EMU_GO)
#undef ZK_EMU_GO
        }
    };
    for (uint32_t b = 0; b < nsegs; b++) emu_run_workgroup(ZKE_THREADS, b, run, nsegs);
}

// per block b in plan order: its counts and where its sequences and literals lie
static void zk_emu_enc_blocks_out(const ZkEncBlock *blocks, uint32_t nb, uint32_t *blk_nseq, uint32_t *blk_nlit, uint32_t *blk_bsz, uint64_t *seq_at, uint64_t *lit_at)
{
    for (uint32_t b = 0; b < nb; b++) {
        blk_nseq[b] = blocks[b].nseq; blk_nlit[b] = blocks[b].nlit; blk_bsz[b] = blocks[b].bsz;
        seq_at[b] = blocks[b].seq_base; lit_at[b] = blocks[b].lit_base;
    }
}
