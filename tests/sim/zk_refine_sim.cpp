// TEST INFRASTRUCTURE -- zk_split_entry (zeekstd_amd/csrc/zk_refine.h), the entry walk of zk_refine_entries, compiled with g++: the lane code
// zk_k_refine_split runs, on the CPU.  tests/helpers/sim_refine.py builds and loads it.
#include "../../zeekstd_amd/csrc/zk_refine.h"

// comp must be readable 8 bytes past c_end (ZK_COMP_PADDING).  starts: nullptr to count, else room for the count.  -> pieces; *stop: 0 or
// why the walk stopped
extern "C" uint32_t zk_sim_split_entry(const uint8_t *comp, uint64_t c_begin, uint64_t c_end, uint64_t *starts, uint32_t *stop)
{
    const ZkSplit s = zk_split_entry(comp, c_begin, c_end, starts);
    *stop = s.stop;
    return s.n;
}
extern "C" uint32_t zk_sim_refine_verdict(uint32_t j, uint32_t code) { return zk_refine_verdict(j, code); }
