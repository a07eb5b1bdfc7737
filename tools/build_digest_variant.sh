#!/bin/bash
# A/B experiments on the digest kernels: builds zeekstd_amd/libzk_<tag>.so from extra -D flags (only zk_digest.hip is recompiled); run a variant
# with ZEEKSTD_AMD_LIB=zeekstd_amd/libzk_<tag>.so python tools/digest_probe.py --digests-only
#   tools/build_digest_variant.sh slab128:-DZKG_SLAB_BYTES=128 slab512:-DZKG_SLAB_BYTES=512 waves4:-DZKG_WAVES_PER_WG=4 direct:-DZKG_DIRECT
set -e
cd "$(dirname "$0")/../zeekstd_amd/csrc"
make -j8 >/dev/null
for spec in "$@"; do
  tag=${spec%%:*}; flags=${spec#*:}
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-function $flags -c zk_digest.hip -o build/var_$tag.o
  objs=$(ls build/*.o | grep -v "zk_digest" | grep -v "/var_" | tr '\n' ' ')
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -Wl,--as-needed -pthread -ldl -o ../libzk_$tag.so build/var_$tag.o $objs
done
