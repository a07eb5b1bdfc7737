"""Level-A batch engine binding (include/zeekstd_amd.h): N frames in, N frames out on one MI355X."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import lib


class ZkError(Exception):
    def __init__(self, code, detail=""):
        self.code = code
        msg = _lib.error_name(code)
        super().__init__(f"{msg} (code {code}){': ' + detail if detail else ''}")


def _u64(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.uint64))


class Dictionary:
    """A zstd dictionary for decoding (zk_dict_create): parsed and validated on the host, no GPU needed.  Bytes that begin with the
    dictionary magic are a formatted dictionary (ZkError -30 when it is damaged), anything else is raw content (id 0)."""

    def __init__(self, data: bytes):
        buf = np.frombuffer(bytes(data), dtype=np.uint8)
        h = C.c_void_p()
        rc = lib.zk_dict_create(buf.ctypes.data if buf.size else None, buf.size, C.byref(h))
        if rc != 0:
            raise ZkError(rc)
        self._h = h

    @property
    def id(self) -> int:
        return int(lib.zk_dict_id(self._h))

    @property
    def content_offset(self) -> int:
        return int(lib.zk_dict_content_offset(self._h))

    def __del__(self):
        if getattr(self, "_h", None):
            lib.zk_dict_free(self._h)
            self._h = None

    @classmethod
    def train(cls, engine, samples, offsets=None, size=112640, **params):
        """A Dictionary of the bytes Engine.train_dictionary makes of the samples (same arguments)."""
        return cls(engine.train_dictionary(samples, offsets, size, **params))


class EncodeDictionary:
    """A dictionary compiled for encoding on one engine (zk_cdict_create; the counterpart of ZSTD_CDict): its content and, for a formatted
    dictionary, the compression side of its tables live on the device.  Made once, used by any number of Engine.encode_frames(dictionary=)
    / encode_frames_dict_dev calls of that engine; it keeps the engine alive."""

    def __init__(self, engine, dictionary):
        h = C.c_void_p()
        rc = lib.zk_cdict_create(engine._h, dictionary._h, C.byref(h))
        if rc != 0:
            engine._raise(rc)
        self._h = h
        self._engine = engine

    @property
    def id(self) -> int:
        return int(lib.zk_cdict_id(self._h))

    def close(self):
        if getattr(self, "_h", None):
            if self._engine._h:
                lib.zk_cdict_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Engine:
    """Owns one GPU's scratch + stream. One thread at a time (like a libzstd context)."""

    def __init__(self, device: int = 0):
        h = C.c_void_p()
        rc = lib.zk_engine_create(device, C.byref(h))
        if rc != 0:
            raise ZkError(rc)
        self._h = h

    def close(self):
        if self._h:
            lib.zk_engine_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def device_name(self) -> str:
        return lib.zk_engine_device_name(self._h).decode()

    def set_dictionary(self, d):
        """Every later decode call of this engine decodes against Dictionary d (zk_engine_set_dictionary); None = none."""
        rc = lib.zk_engine_set_dictionary(self._h, d._h if d is not None else None)
        if rc != 0:
            self._raise(rc)

    def set_profiling(self, on: bool):
        rc = lib.zk_engine_set_profiling(self._h, int(on))
        if rc != 0:
            self._raise(rc)

    def set_fse_kernel(self, mode: int):
        """0 = by batch size, 1 = one lane per block, 2 = a quad of lanes per block (own-table blocks; same results)."""
        rc = lib.zk_engine_set_fse_kernel(self._h, int(mode))
        if rc != 0:
            self._raise(rc)

    CHOICES = {"reset": 0, "fse_own": 1, "fse_shared": 2, "exec_lanes": 3, "exec_ring": 4, "xxh64": 5, "small_path": 6,
               "pipe_contexts": 7, "pipe_chunk_mib": 8, "exec_resident": 9, "exec_seg": 10, "seg_kib": 11, "seg_fill": 12,
               "entropy": 13, "range_pass_mib": 14, "enc_dense_slice_kib": 15, "enc_dict_slice_kib": 16, "enc_plan": 17, "train_trial_kib": 18,
               "cdc_slice_kib": 19, "dedup_key_bits": 20, "dedup_slice_kib": 21, "dedup_pass_kib": 22, "compact_slice_kib": 23}

    def frame_content_sizes(self, comp: bytes, c_off, first=0, count=None):
        """zk_frame_content_sizes: the decompressed sizes of frames nobody holds seek entries for (header walk + sequence walks on the device,
        no output) -> (uint64 array, int32 status array: 0 or -ZSTD_ErrorCode per frame)"""
        c = _u64(c_off)
        count = len(c) - 1 - first if count is None else count
        src = np.frombuffer(bytes(comp) + b"\0" * 8, np.uint8)
        sizes = np.zeros(max(count, 1), np.uint64)
        st = np.zeros(max(count, 1), np.int32)
        rc = lib.zk_frame_content_sizes(self._h, src.ctypes.data, len(comp), c.ctypes.data, first, count, sizes.ctypes.data, st.ctypes.data)
        if rc != 0:
            self._raise(rc)
        return sizes[:count], st[:count]

    def refine_entries(self, comp: bytes, c_off, d_off=None, raise_on_error=False):
        """zk_refine_entries: the table (c_off, d_off) of `comp` refined to one entry per frame.  An entry may be any chain of Zstandard
        and skippable frames; d_off=None: nobody knows the sizes (a plain multi-frame stream: c_off = [0, len(comp)]).
        -> (c_off', d_off', entry_of, status): uint64 prefix sums of the refined table, the input entry each refined entry came from, and
        per INPUT entry 0 or -ZSTD_ErrorCode (a bad entry stays one refined entry)."""
        c = _u64(c_off)
        d = _u64(d_off) if d_off is not None else None
        n = len(c) - 1
        src = np.frombuffer(bytes(comp) + b"\0" * 8, np.uint8)
        st = np.zeros(max(n, 1), np.int32)
        n_out = C.c_uint32()
        args = (self._h, src.ctypes.data, len(comp), c.ctypes.data, d.ctypes.data if d is not None else None, n)
        rc = lib.zk_refine_entries(*args, None, None, None, 0, C.byref(n_out), st.ctypes.data)
        if rc != -70 and rc != 0:
            self._raise(rc)
        m = n_out.value
        co, do, eo = np.zeros(m + 1, np.uint64), np.zeros(m + 1, np.uint64), np.zeros(max(m, 1), np.uint32)
        if m:
            rc = lib.zk_refine_entries(*args, co.ctypes.data, do.ctypes.data, eo.ctypes.data, m, C.byref(n_out), st.ctypes.data)
            if rc <= -1000 or (rc != 0 and raise_on_error):
                self._raise(rc)
        return co, do, eo[:m], st[:n]

    def refine_entries_dev(self, d_comp, comp_size, d_c_off, d_d_off, n_entries, d_c_out, d_d_out, d_entry_of, out_cap, d_status, stream=None):
        """zk_refine_entries_dev on device buffers (torch tensors or raw ints; d_d_off, d_c_out, d_d_out, d_entry_of may be None)
        -> (return code, number of refined entries)"""
        opt = lambda t: self._ptr(t) if t is not None else None
        n_out = C.c_uint32()
        rc = lib.zk_refine_entries_dev(self._h, self._ptr(d_comp), comp_size, self._ptr(d_c_off), opt(d_d_off), n_entries,
                                       opt(d_c_out), opt(d_d_out), opt(d_entry_of), out_cap, C.byref(n_out), self._ptr(d_status), stream)
        if rc <= -1000 and rc != -2003:
            self._raise(rc)
        return rc, n_out.value

    def checksums_followed(self):
        """Frames of the last finished decode that zk_k_xxh64_follow verified beside the executor (zk_engine_checksums_followed)."""
        return int(lib.zk_engine_checksums_followed(self._h))

    def entropy_fused(self):
        """Whether the last finished decode ran literals and sequences in one kernel, zk_k_entropy_frame (zk_engine_entropy_fused)."""
        return bool(lib.zk_engine_entropy_fused(self._h))

    def set_kernel_choice(self, **kw):
        """Pins kernel variants (zk_engine_set_kernel_choice): e.g. set_kernel_choice(fse_shared=2, exec_lanes=256, xxh64=2) runs the
        large-batch kernels on whatever is decoded next; set_kernel_choice(reset=0) returns to "by batch shape"."""
        for key, value in kw.items():
            rc = lib.zk_engine_set_kernel_choice(self._h, self.CHOICES[key], int(value))
            if rc != 0:
                self._raise(rc)

    def kernel_times(self):
        """{kernel name: ms} of the last decode/encode call (profiling must be on)."""
        n = lib.zk_engine_kernel_count()
        ms = (C.c_float * n)()
        lib.zk_engine_kernel_times(self._h, ms, n)
        return {lib.zk_engine_kernel_name(k).decode(): float(ms[k]) for k in range(n) if ms[k] > 0}

    def _raise(self, rc):
        raise ZkError(rc, lib.zk_engine_last_hip_error(self._h).decode() if rc == -2001 else "")

    # ---- host-pointer entry points
    def decode_frames(self, comp, c_off, d_off, first=0, count=None, verify=True, raise_on_error=True, prefix=None):
        """Returns (bytes of frames [first, first+count), per-frame status array).
        prefix: raw-content prefix every frame was compressed against (patch mode)."""
        comp = np.frombuffer(comp, dtype=np.uint8) if not isinstance(comp, np.ndarray) else comp
        c_off, d_off = _u64(c_off), _u64(d_off)
        if count is None:
            count = len(c_off) - 1 - first
        out_len = int(d_off[first + count] - d_off[first])
        out = np.empty(max(out_len, 1), dtype=np.uint8)
        status = np.zeros(max(count, 1), dtype=np.int32)
        if prefix:
            pre = np.frombuffer(bytes(prefix), dtype=np.uint8)
            rc = lib.zk_decode_frames_prefix(self._h, comp.ctypes.data, comp.size, c_off.ctypes.data, d_off.ctypes.data,
                                             first, count, pre.ctypes.data, pre.size, out.ctypes.data, out_len, int(verify),
                                             status.ctypes.data)
        else:
            rc = lib.zk_decode_frames(self._h, comp.ctypes.data, comp.size, c_off.ctypes.data, d_off.ctypes.data,
                                      first, count, out.ctypes.data, out_len, int(verify), status.ctypes.data)
        if rc != 0 and (raise_on_error or rc <= -1000):
            self._raise(rc)
        return out[:out_len].tobytes(), status[:count]

    def encode_frames(self, data, frame_size=0x200000, level=1, checksum=False, prefix=None, dictionary=None):
        """Returns (compressed payload bytes, [(c_size, d_size), ...]) -- one zstd frame per frame_size bytes.
        prefix: raw-content prefix referenced at the start of every frame (patch mode).
        dictionary: an EncodeDictionary of this engine (zk_encode_frames_dict); not together with a prefix."""
        data = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else data
        n = int(data.size)
        nf = max(1, -(-n // frame_size))
        if dictionary is not None and prefix:
            raise ValueError("a prefix and a dictionary exclude each other at this level")
        cap = int(lib.zk_compress_bound_dict(n, frame_size) if dictionary is not None else lib.zk_compress_bound(n, frame_size))
        out = np.empty(cap, dtype=np.uint8)
        cs = np.zeros(nf, np.uint32)
        ds = np.zeros(nf, np.uint32)
        nfo = C.c_uint32()
        wr = C.c_uint64()
        if dictionary is not None:
            rc = lib.zk_encode_frames_dict(self._h, data.ctypes.data if n else None, n, frame_size, level, int(checksum), dictionary._h,
                                           out.ctypes.data, cap, cs.ctypes.data, ds.ctypes.data, nf, C.byref(nfo), C.byref(wr))
        elif prefix:
            pre = np.frombuffer(bytes(prefix), dtype=np.uint8)
            rc = lib.zk_encode_frames_prefix(self._h, data.ctypes.data if n else None, n, frame_size, level, int(checksum),
                                             pre.ctypes.data, pre.size, out.ctypes.data, cap, cs.ctypes.data, ds.ctypes.data, nf,
                                             C.byref(nfo), C.byref(wr))
        else:
            rc = lib.zk_encode_frames(self._h, data.ctypes.data if n else None, n, frame_size, level, int(checksum),
                                      out.ctypes.data, cap, cs.ctypes.data, ds.ctypes.data, nf, C.byref(nfo), C.byref(wr))
        if rc != 0:
            self._raise(rc)
        return out[:wr.value].tobytes(), list(zip(cs[:nfo.value].tolist(), ds[:nfo.value].tolist()))

    def encode_frames_dev(self, d_src, n, frame_size, level, checksum, d_dst, dst_cap, d_c_sizes=None, d_d_sizes=None, stream=None):
        nfo = C.c_uint32()
        wr = C.c_uint64()
        rc = lib.zk_encode_frames_dev(self._h, self._ptr(d_src), n, frame_size, level, int(checksum), self._ptr(d_dst), dst_cap,
                                      self._ptr(d_c_sizes) if d_c_sizes is not None else None,
                                      self._ptr(d_d_sizes) if d_d_sizes is not None else None, C.byref(nfo), C.byref(wr), stream)
        if rc != 0:
            self._raise(rc)
        return nfo.value, wr.value

    def encode_frames_dict_dev(self, d_src, n, frame_size, level, checksum, dictionary, d_dst, dst_cap, d_c_sizes=None, d_d_sizes=None, stream=None):
        """zk_encode_frames_dict_dev: device tensors in and out, `dictionary` an EncodeDictionary of this engine (None is refused by the
        library).  Returns (frames, bytes written)."""
        nfo = C.c_uint32()
        wr = C.c_uint64()
        rc = lib.zk_encode_frames_dict_dev(self._h, self._ptr(d_src), n, frame_size, level, int(checksum),
                                           dictionary._h if dictionary is not None else None, self._ptr(d_dst), dst_cap,
                                           self._ptr(d_c_sizes) if d_c_sizes is not None else None,
                                           self._ptr(d_d_sizes) if d_d_sizes is not None else None, C.byref(nfo), C.byref(wr), stream)
        if rc != 0:
            self._raise(rc)
        return nfo.value, wr.value

    def encode_frame_list(self, data, offsets, level=1, checksum=False, prefix=None, dictionary=None):
        """zk_encode_frame_list: one zstd frame per entry of `offsets` (len(frames) + 1 non-decreasing prefix sums into data; the array the
        decode calls take as d_off).  Returns (compressed payload bytes, [(c_size, d_size), ...]).  prefix / dictionary as encode_frames."""
        data = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else data
        off = _u64(offsets)
        count = max(len(off) - 1, 0)
        if dictionary is not None and prefix:
            raise ValueError("a prefix and a dictionary exclude each other at this level")
        n = int(off[count] - off[0]) if count and off[count] >= off[0] else 0
        cap = int(lib.zk_compress_bound_list(n, count, int(dictionary is not None)))
        out = np.empty(max(cap, 1), dtype=np.uint8)
        cs = np.zeros(max(count, 1), np.uint32)
        ds = np.zeros(max(count, 1), np.uint32)
        wr = C.c_uint64()
        pre = np.frombuffer(bytes(prefix), dtype=np.uint8) if prefix else None
        rc = lib.zk_encode_frame_list(self._h, data.ctypes.data if data.size else None, off.ctypes.data, count, level, int(checksum),
                                      pre.ctypes.data if pre is not None else None, pre.size if pre is not None else 0,
                                      dictionary._h if dictionary is not None else None, out.ctypes.data, cap, cs.ctypes.data, ds.ctypes.data,
                                      C.byref(wr))
        if rc != 0:
            self._raise(rc)
        return out[:wr.value].tobytes(), list(zip(cs[:count].tolist(), ds[:count].tolist()))

    def encode_frame_list_dev(self, d_src, d_off, count, level, checksum, d_dst, dst_cap, d_c_sizes=None, d_d_sizes=None, d_prefix=None,
                              prefix_len=0, dictionary=None, stream=None):
        """zk_encode_frame_list_dev: device tensors in and out, d_off = count + 1 uint64 prefix sums on the device.  Returns bytes written."""
        wr = C.c_uint64()
        rc = lib.zk_encode_frame_list_dev(self._h, self._ptr(d_src) if d_src is not None else None, self._ptr(d_off) if d_off is not None else None,
                                          count, level, int(checksum), self._ptr(d_prefix) if d_prefix is not None else None, prefix_len,
                                          dictionary._h if dictionary is not None else None, self._ptr(d_dst) if d_dst is not None else None, dst_cap,
                                          self._ptr(d_c_sizes) if d_c_sizes is not None else None,
                                          self._ptr(d_d_sizes) if d_d_sizes is not None else None, C.byref(wr), stream)
        if rc != 0:
            self._raise(rc)
        return wr.value

    @staticmethod
    def _chunk_frames(n, avg_size, min_size):
        """n / min + 1: no chain has more cuts (the defaults as the library resolves them)"""
        return n // (min_size or (avg_size or 1 << 21) // 4 or 1) + 1

    def chunk_boundaries(self, data, avg_size=0, min_size=0, max_size=0):
        """zk_chunk_boundaries: content-defined frame boundaries of `data` (the rule of include/zeekstd_amd.h; 0 = the default).  Returns the
        count + 1 offsets as an np.uint64 array: what encode_frame_list and the decode calls take."""
        data = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else data
        n = int(data.size)
        par = _lib.ChunkParams(min_size, avg_size, max_size, 0)
        count = C.c_uint32()
        cap = self._chunk_frames(n, avg_size, min_size)
        off = np.zeros(cap + 1, np.uint64)
        rc = lib.zk_chunk_boundaries(self._h, data.ctypes.data if n else None, n, C.byref(par), off.ctypes.data, cap, C.byref(count))
        if rc != 0:
            self._raise(rc)
        return off[:count.value + 1].copy()

    def chunk_boundaries_dev(self, d_src, n, avg_size=0, min_size=0, max_size=0, stream=None):
        """zk_chunk_boundaries_dev: the source is a device tensor (or raw pointer); returns a device tensor of count + 1 offsets (int64: the
        bits of the uint64 array zk_encode_frame_list_dev takes; a view of an array of n / min + 2 entries)."""
        import torch
        par = _lib.ChunkParams(min_size, avg_size, max_size, 0)
        count = C.c_uint32()
        cap = self._chunk_frames(n, avg_size, min_size)
        off = torch.zeros(cap + 1, dtype=torch.int64, device=d_src.device if hasattr(d_src, "device") else "cuda")
        rc = lib.zk_chunk_boundaries_dev(self._h, self._ptr(d_src) if d_src is not None and n else None, n, C.byref(par), off.data_ptr(), cap,
                                         C.byref(count), stream)
        if rc != 0:
            self._raise(rc)
        return off[:count.value + 1]

    def encode_chunked(self, data, avg_size=0, min_size=0, max_size=0, level=1, checksum=False, prefix=None, dictionary=None):
        """zk_encode_chunked: content-defined boundaries, then one zstd frame per piece (encode_frame_list on those offsets).  Returns
        (compressed payload bytes, np.uint64 offsets, np.uint32 c_sizes).  prefix / dictionary as encode_frames."""
        data = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else data
        n = int(data.size)
        if dictionary is not None and prefix:
            raise ValueError("a prefix and a dictionary exclude each other at this level")
        par = _lib.ChunkParams(min_size, avg_size, max_size, 0)
        cap = int(lib.zk_compress_bound_chunked(n, C.byref(par), int(dictionary is not None)))
        if cap == 0:
            self._raise(-2003)
        frames = self._chunk_frames(n, avg_size, min_size)
        out = np.empty(cap, dtype=np.uint8)
        off = np.zeros(frames + 1, np.uint64)
        cs = np.zeros(frames, np.uint32)
        ds = np.zeros(frames, np.uint32)
        nfo = C.c_uint32()
        wr = C.c_uint64()
        pre = np.frombuffer(bytes(prefix), dtype=np.uint8) if prefix else None
        rc = lib.zk_encode_chunked(self._h, data.ctypes.data if n else None, n, C.byref(par), level, int(checksum),
                                   pre.ctypes.data if pre is not None else None, pre.size if pre is not None else 0,
                                   dictionary._h if dictionary is not None else None, out.ctypes.data, cap, off.ctypes.data, frames,
                                   cs.ctypes.data, ds.ctypes.data, C.byref(nfo), C.byref(wr))
        if rc != 0:
            self._raise(rc)
        return out[:wr.value].tobytes(), off[:nfo.value + 1].copy(), cs[:nfo.value].copy()

    def encode_chunked_dev(self, d_src, n, d_dst, dst_cap, d_off, off_cap, avg_size=0, min_size=0, max_size=0, level=1, checksum=False,
                           d_c_sizes=None, d_d_sizes=None, d_prefix=None, prefix_len=0, dictionary=None, stream=None):
        """zk_encode_chunked_dev: device tensors in and out; d_off receives the offsets (off_cap + 1 uint64 entries), d_c_sizes / d_d_sizes
        off_cap uint32 entries each.  Returns (frames, bytes written)."""
        opt = lambda t: self._ptr(t) if t is not None else None
        par = _lib.ChunkParams(min_size, avg_size, max_size, 0)
        nfo = C.c_uint32()
        wr = C.c_uint64()
        rc = lib.zk_encode_chunked_dev(self._h, opt(d_src), n, C.byref(par), level, int(checksum), opt(d_prefix), prefix_len,
                                       dictionary._h if dictionary is not None else None, opt(d_dst), dst_cap, opt(d_off), off_cap,
                                       opt(d_c_sizes), opt(d_d_sizes), C.byref(nfo), C.byref(wr), stream)
        if rc != 0:
            self._raise(rc)
        return nfo.value, wr.value

    def dedup_frames(self, data, offsets):
        """zk_dedup_frames: which frames of `data` (cut by `offsets`, as encode_frame_list takes them) are byte-identical.  Returns
        (ref, ids, uniq) as np.uint32 arrays: ref[i] the first frame with frame i's bytes, uniq the frames with ref[i] == i in ascending
        order, ids[i] the position of ref[i] in uniq (what decode_frame_list_dev takes as d_ids for an archive of the uniq frames)."""
        data = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else data
        off = _u64(offsets)
        count = max(len(off) - 1, 0)
        ref, ids, uniq = (np.zeros(max(count, 1), np.uint32) for _ in range(3))
        nu = C.c_uint32()
        rc = lib.zk_dedup_frames(self._h, data.ctypes.data if data.size else None, off.ctypes.data, count, ref.ctypes.data, ids.ctypes.data,
                                 uniq.ctypes.data, C.byref(nu))
        if rc != 0:
            self._raise(rc)
        return ref[:count], ids[:count], uniq[:nu.value]

    def dedup_frames_dev(self, d_src, d_off, count, d_ref=None, d_ids=None, d_uniq=None, stream=None):
        """zk_dedup_frames_dev: device tensors (or raw pointers) in and out; d_ref / d_ids / d_uniq: uint32 arrays of `count` entries, any
        of them None.  Returns n_unique."""
        opt = lambda t: self._ptr(t) if t is not None else None
        nu = C.c_uint32()
        rc = lib.zk_dedup_frames_dev(self._h, opt(d_src), opt(d_off), count, opt(d_ref), opt(d_ids), opt(d_uniq), C.byref(nu), stream)
        if rc != 0:
            self._raise(rc)
        return nu.value

    def encode_dedup_dev(self, d_src, d_off, count, level, checksum, d_dst, dst_cap, d_ids=None, d_uniq=None, d_c_sizes=None, d_d_sizes=None,
                         d_prefix=None, prefix_len=0, dictionary=None, stream=None):
        """zk_encode_dedup_dev: every distinct frame of the list encoded once, device tensors in and out (d_ids / d_uniq / d_c_sizes /
        d_d_sizes: uint32, `count` entries each).  Returns (n_unique, bytes written)."""
        opt = lambda t: self._ptr(t) if t is not None else None
        nu = C.c_uint32()
        wr = C.c_uint64()
        rc = lib.zk_encode_dedup_dev(self._h, opt(d_src), opt(d_off), count, level, int(checksum), opt(d_prefix), prefix_len,
                                     dictionary._h if dictionary is not None else None, opt(d_dst), dst_cap, opt(d_ids), opt(d_uniq),
                                     opt(d_c_sizes), opt(d_d_sizes), C.byref(nu), C.byref(wr), stream)
        if rc != 0:
            self._raise(rc)
        return nu.value, wr.value

    def encode_dedup(self, data, offsets=None, avg_size=0, min_size=0, max_size=0, level=1, checksum=False, prefix=None, dictionary=None):
        """zk_encode_dedup: one zstd frame per DISTINCT frame of `data`.  offsets: the frames (as encode_frame_list takes them); None: the
        content-defined boundaries of chunk_boundaries(data, avg_size, min_size, max_size) first.  Returns (compressed payload bytes of the
        unique frames, np.uint64 offsets of all frames, np.uint32 c_sizes and d_sizes of the unique frames, np.uint32 ids: frame i of the
        input is archive frame ids[i]).  prefix / dictionary as encode_frames."""
        data = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else data
        if dictionary is not None and prefix:
            raise ValueError("a prefix and a dictionary exclude each other at this level")
        off = self.chunk_boundaries(data, avg_size, min_size, max_size) if offsets is None else _u64(offsets)
        count = max(len(off) - 1, 0)
        n = int(off[count] - off[0]) if count and off[count] >= off[0] else 0
        cap = int(lib.zk_compress_bound_list(n, count, int(dictionary is not None)))
        out = np.empty(max(cap, 1), dtype=np.uint8)
        cs, ds, ids, uniq = (np.zeros(max(count, 1), np.uint32) for _ in range(4))
        nu = C.c_uint32()
        wr = C.c_uint64()
        pre = np.frombuffer(bytes(prefix), dtype=np.uint8) if prefix else None
        rc = lib.zk_encode_dedup(self._h, data.ctypes.data if data.size else None, off.ctypes.data, count, level, int(checksum),
                                 pre.ctypes.data if pre is not None else None, pre.size if pre is not None else 0,
                                 dictionary._h if dictionary is not None else None, out.ctypes.data, cap, ids.ctypes.data, uniq.ctypes.data,
                                 cs.ctypes.data, ds.ctypes.data, C.byref(nu), C.byref(wr))
        if rc != 0:
            self._raise(rc)
        return out[:wr.value].tobytes(), off, cs[:nu.value].copy(), ds[:nu.value].copy(), ids[:count].copy()

    def frame_keys(self, data, offsets):
        """zk_frame_keys: the 64-bit key of every frame of `data` (cut by `offsets`) as a dedup index stores it -> np.uint64 array"""
        data = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else data
        off = _u64(offsets)
        count = max(len(off) - 1, 0)
        keys = np.zeros(max(count, 1), np.uint64)
        rc = lib.zk_frame_keys(self._h, data.ctypes.data if data.size else None, off.ctypes.data, count, keys.ctypes.data)
        if rc != 0:
            self._raise(rc)
        return keys[:count]

    def frame_keys_dev(self, d_src, d_off, count, d_keys, stream=None):
        """zk_frame_keys_dev: device tensors (or raw pointers); d_keys: count uint64 words, 8-byte aligned"""
        opt = lambda t: self._ptr(t) if t is not None else None
        rc = lib.zk_frame_keys_dev(self._h, opt(d_src), opt(d_off), count, opt(d_keys), stream)
        if rc != 0:
            self._raise(rc)

    DIGESTS = {"sha256": 1, "blake2s-tree": 2}              # ZK_DIGEST_SHA256, ZK_DIGEST_BLAKE2S_TREE

    @classmethod
    def _digest_algo(cls, algo):
        if algo not in cls.DIGESTS:
            raise ValueError("algo must be one of %s" % ", ".join(sorted(cls.DIGESTS)))
        return cls.DIGESTS[algo]

    def frame_digests(self, data, offsets, algo="sha256"):
        """zk_frame_digests: the digest of every frame of `data` (cut by `offsets`), algo "sha256" or "blake2s-tree" (the tree of
        include/zeekstd_amd.h, leaves of 4096 bytes) -> np.uint8[count, 32], a row's bytes in the order hexdigest() prints them"""
        code = self._digest_algo(algo)
        data = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else data
        off = _u64(offsets)
        count = max(len(off) - 1, 0)
        out = np.zeros((max(count, 1), 32), np.uint8)
        rc = lib.zk_frame_digests(self._h, code, data.ctypes.data if data.size else None, off.ctypes.data, count, out.ctypes.data)
        if rc != 0:
            self._raise(rc)
        return out[:count]

    def frame_digests_dev(self, d_src, d_off, count, d_digests, algo="sha256", stream=None):
        """zk_frame_digests_dev: device tensors (or raw pointers); d_digests: 32 * count bytes, 4-byte aligned"""
        opt = lambda t: self._ptr(t) if t is not None else None
        rc = lib.zk_frame_digests_dev(self._h, self._digest_algo(algo), opt(d_src), opt(d_off), count, opt(d_digests), stream)
        if rc != 0:
            self._raise(rc)

    def archive_digests_dev(self, d_comp, comp_size, d_c_off, d_d_off, first, count, d_digests, algo="sha256", stream=None):
        """zk_archive_digests_dev: the digests of the decoded content of archive frames [first, first + count) -> d_digests (32 * count bytes,
        4-byte aligned).  Returns 0 or -(code) of a frame that failed to decode or verify"""
        opt = lambda t: self._ptr(t) if t is not None else None
        rc = lib.zk_archive_digests_dev(self._h, self._digest_algo(algo), opt(d_comp), comp_size, opt(d_c_off), opt(d_d_off), first, count, opt(d_digests), stream)
        if rc <= -1000:
            self._raise(rc)
        return rc

    def dedup_against_dev(self, index, d_comp, comp_size, d_c_off, d_d_off, n_frames, d_src, d_off, count, d_ids=None, d_fresh=None, stream=None):
        """zk_dedup_against_dev: which frames of the list the archive (d_comp, d_c_off, d_d_off, n_frames; known to `index`) already holds.
        d_ids / d_fresh: uint32 device arrays of `count` entries, or None.  Returns n_fresh."""
        opt = lambda t: self._ptr(t) if t is not None else None
        nf = C.c_uint32()
        rc = lib.zk_dedup_against_dev(self._h, index._h, opt(d_comp), comp_size, opt(d_c_off), opt(d_d_off), n_frames, opt(d_src), opt(d_off), count,
                                      opt(d_ids), opt(d_fresh), C.byref(nf), stream)
        if rc != 0:
            self._raise(rc)
        return nf.value

    def encode_dedup_against_dev(self, index, d_comp, comp_size, d_c_off, d_d_off, n_frames, d_src, d_off, count, level, checksum, d_dst, dst_cap,
                                 d_ids=None, d_fresh=None, d_c_sizes=None, d_d_sizes=None, dictionary=None, stream=None):
        """zk_encode_dedup_against_dev: the frames of the list the archive does not hold yet, each encoded once; `index` learns them.
        Returns (n_fresh, bytes written)."""
        opt = lambda t: self._ptr(t) if t is not None else None
        nf = C.c_uint32()
        wr = C.c_uint64()
        rc = lib.zk_encode_dedup_against_dev(self._h, index._h, opt(d_comp), comp_size, opt(d_c_off), opt(d_d_off), n_frames, opt(d_src), opt(d_off), count,
                                             level, int(checksum), dictionary._h if dictionary is not None else None, opt(d_dst), dst_cap, opt(d_ids),
                                             opt(d_fresh), opt(d_c_sizes), opt(d_d_sizes), C.byref(nf), C.byref(wr), stream)
        if rc != 0:
            self._raise(rc)
        return nf.value, wr.value

    def mark_frames_dev(self, d_ids, count, n_frames, d_live, stream=None):
        """zk_mark_frames_dev: live[ids[i]] = 1 for `count` uint32 ids (device tensors or raw pointers); d_live: n_frames uint8 flags, zeroed by
        the caller before the first snapshot it keeps is marked"""
        rc = lib.zk_mark_frames_dev(self._h, self._ptr(d_ids), count, n_frames, self._ptr(d_live), stream)
        if rc != 0:
            self._raise(rc)

    def compact_archive_dev(self, d_comp, comp_size, d_c_off, d_d_off, n_frames, d_live, d_dst, dst_cap, d_c_off_out=None, d_d_off_out=None,
                            d_remap=None, stream=None, raise_on_error=True):
        """zk_compact_archive_dev: the frames with live[s] != 0, in order and back to back in d_dst (d_dst may be d_comp: in place).  d_c_off_out /
        d_d_off_out: uint64 arrays of n_frames + 1 entries, d_remap: uint32 of n_frames, or None.  Returns (n_kept, written); with
        raise_on_error=False (rc, n_kept, written)."""
        opt = lambda t: self._ptr(t) if t is not None else None
        nk = C.c_uint32()
        wr = C.c_uint64()
        rc = lib.zk_compact_archive_dev(self._h, opt(d_comp), comp_size, opt(d_c_off), opt(d_d_off), n_frames, opt(d_live), opt(d_dst), dst_cap,
                                        opt(d_c_off_out), opt(d_d_off_out), opt(d_remap), C.byref(nk), C.byref(wr), stream)
        if not raise_on_error:
            return rc, nk.value, wr.value
        if rc != 0:
            self._raise(rc)
        return nk.value, wr.value

    def remap_ids_dev(self, d_remap, n_frames, d_ids, count, d_ids_out=None, stream=None):
        """zk_remap_ids_dev: ids_out[i] = remap[ids[i]] (d_ids_out None: in place)"""
        rc = lib.zk_remap_ids_dev(self._h, self._ptr(d_remap), n_frames, self._ptr(d_ids), count, self._ptr(d_ids_out if d_ids_out is not None else d_ids), stream)
        if rc != 0:
            self._raise(rc)

    @staticmethod
    def _train_params(k, d, f, level, dict_id, raw_content):
        return _lib.TrainParams(k, d, f, level, dict_id, _lib.TRAIN_RAW_CONTENT if raw_content else 0)

    def train_dictionary(self, samples, offsets=None, size=112640, k=0, d=0, f=0, level=0, dict_id=0, raw_content=False, report=False):
        """zk_train_dictionary: a zstd dictionary of at most `size` bytes trained on the device.  samples: a list of bytes objects, or one
        buffer with `offsets` (len(samples) + 1 non-decreasing prefix sums into it).  k / d / f / level / dict_id: zk_train_params, 0 = the
        default; raw_content: the content alone (ZK_TRAIN_RAW_CONTENT).  Returns the dictionary's bytes; report=True: (bytes, dict of the
        zk_train_report fields)."""
        if offsets is None:
            sizes = [len(x) for x in samples]
            data = np.frombuffer(b"".join(bytes(x) for x in samples), dtype=np.uint8)
            off = np.zeros(len(sizes) + 1, np.uint64)
            off[1:] = np.cumsum(sizes, dtype=np.uint64)
        else:
            data = np.frombuffer(samples, dtype=np.uint8) if not isinstance(samples, np.ndarray) else samples
            off = _u64(offsets)
        out = np.empty(max(int(size), 1), np.uint8)
        wr = C.c_size_t()
        rep = _lib.TrainReport()
        par = self._train_params(k, d, f, level, dict_id, raw_content)
        rc = lib.zk_train_dictionary(self._h, data.ctypes.data if data.size else None, off.ctypes.data, max(len(off) - 1, 0), C.byref(par),
                                     out.ctypes.data, int(size), C.byref(wr), C.byref(rep))
        if rc != 0:
            self._raise(rc)
        got = out[:wr.value].tobytes()
        return (got, {n: int(getattr(rep, n)) for n, _ in rep._fields_}) if report else got

    def train_dictionary_dev(self, d_samples, d_off, count, size=112640, k=0, d=0, f=0, level=0, dict_id=0, raw_content=False, report=False, stream=None):
        """zk_train_dictionary_dev: the samples and their count + 1 uint64 offsets are device tensors (or raw pointers); the dictionary's
        bytes come back on the host as from train_dictionary."""
        out = np.empty(max(int(size), 1), np.uint8)
        wr = C.c_size_t()
        rep = _lib.TrainReport()
        par = self._train_params(k, d, f, level, dict_id, raw_content)
        rc = lib.zk_train_dictionary_dev(self._h, self._ptr(d_samples) if d_samples is not None else None, self._ptr(d_off) if d_off is not None else None,
                                         count, C.byref(par), out.ctypes.data, int(size), C.byref(wr), C.byref(rep), stream)
        if rc != 0:
            self._raise(rc)
        got = out[:wr.value].tobytes()
        return (got, {n: int(getattr(rep, n)) for n, _ in rep._fields_}) if report else got

    def xxh64_frames(self, data, off):
        data = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else data
        off = _u64(off)
        n = len(off) - 1
        out = np.zeros(max(n, 1), dtype=np.uint64)
        rc = lib.zk_xxh64_frames(self._h, data.ctypes.data if data.size else None, off.ctypes.data, n, out.ctypes.data)
        if rc != 0:
            self._raise(rc)
        return out[:n]

    # ---- device-pointer entry points (torch tensors or raw ints)
    @staticmethod
    def _ptr(t):
        return t.data_ptr() if hasattr(t, "data_ptr") else int(t)

    def decode_frames_dev(self, d_comp, comp_size, d_c_off, d_d_off, first, count, d_dst, dst_cap, verify=True,
                          d_status=None, stream=None):
        rc = lib.zk_decode_frames_dev(self._h, self._ptr(d_comp), comp_size, self._ptr(d_c_off), self._ptr(d_d_off),
                                      first, count, self._ptr(d_dst), dst_cap, int(verify),
                                      self._ptr(d_status) if d_status is not None else None, stream)
        if rc <= -1000:
            self._raise(rc)
        return rc

    def decode_frames_prefix_dev(self, d_comp, comp_size, d_c_off, d_d_off, first, count, d_prefix, prefix_len, d_dst, dst_cap,
                                 verify=True, d_status=None, stream=None):
        rc = lib.zk_decode_frames_prefix_dev(self._h, self._ptr(d_comp), comp_size, self._ptr(d_c_off), self._ptr(d_d_off),
                                             first, count, self._ptr(d_prefix) if prefix_len else None, prefix_len,
                                             self._ptr(d_dst), dst_cap, int(verify),
                                             self._ptr(d_status) if d_status is not None else None, stream)
        if rc <= -1000:
            self._raise(rc)
        return rc

    def decode_submit_dev(self, d_comp, comp_size, d_c_off, d_d_off, first, count, d_dst, dst_cap, verify=True, d_status=None):
        """Enqueue a batch on one of the engine's two decode contexts; returns the slot to pass to decode_wait()."""
        slot = C.c_int(-1)
        rc = lib.zk_decode_submit_dev(self._h, self._ptr(d_comp), comp_size, self._ptr(d_c_off), self._ptr(d_d_off),
                                      first, count, self._ptr(d_dst), dst_cap, int(verify),
                                      self._ptr(d_status) if d_status is not None else None, C.byref(slot))
        if rc != 0:
            if rc <= -1000:
                self._raise(rc)
            raise RuntimeError(f"zk_decode_submit_dev: {rc}")
        return slot.value

    def decode_wait(self, slot):
        rc = lib.zk_decode_wait(self._h, int(slot))
        if rc <= -1000:
            self._raise(rc)
        return rc

    def decode_frame_list_dev(self, d_comp, comp_size, d_c_off, d_d_off, d_ids, d_out_off, count, d_dst, dst_cap, verify=True,
                              d_status=None, stream=None):
        """Random-access batch: archive frames d_ids[i] -> d_dst + d_out_off[i] (all device-resident)."""
        rc = lib.zk_decode_frame_list_dev(self._h, self._ptr(d_comp), comp_size, self._ptr(d_c_off), self._ptr(d_d_off),
                                          self._ptr(d_ids), self._ptr(d_out_off), count, self._ptr(d_dst), dst_cap, int(verify),
                                          self._ptr(d_status) if d_status is not None else None, stream)
        if rc <= -1000:
            self._raise(rc)
        return rc

    def read_ranges_dev(self, d_comp, comp_size, d_c_off, d_d_off, n_frames, d_offs, d_lens, d_dst_off, count, d_dst, dst_cap,
                        verify=True, d_status=None, stream=None):
        """Batched reads (zk_read_ranges_dev): bytes [d_offs[i], d_offs[i] + d_lens[i]) of the decompressed stream -> d_dst + d_dst_off[i]
        (d_dst_off None: packed in list order); everything device-resident, uint64 arrays.  Returns 0 or the first failing range's status."""
        rc = lib.zk_read_ranges_dev(self._h, self._ptr(d_comp), comp_size, self._ptr(d_c_off), self._ptr(d_d_off), n_frames,
                                    self._ptr(d_offs), self._ptr(d_lens), self._ptr(d_dst_off) if d_dst_off is not None else None, count,
                                    self._ptr(d_dst) if d_dst is not None else None, dst_cap, int(verify),
                                    self._ptr(d_status) if d_status is not None else None, stream)
        if rc <= -1000 and rc != -1001:
            self._raise(rc)
        return rc

    def read_view_ranges_dev(self, d_comp, comp_size, d_c_off, d_d_off, n_frames, d_view_ids, d_view_off, view_count, d_offs, d_lens, d_dst_off, count,
                             d_dst, dst_cap, verify=True, d_status=None, stream=None):
        """Batched reads of a view (zk_read_view_ranges_dev): the view's stream is the decoded archive frames d_view_ids[j] (uint32) laid out by
        d_view_off (uint64, view_count + 1) -- the ids / offsets pair the dedup calls return --; bytes [d_offs[i], d_offs[i] + d_lens[i]) of it ->
        d_dst + d_dst_off[i] (None: packed in list order).  Every archive frame is decoded at most once.  Returns 0 or the first failing range's
        status; a view that does not fit the archive raises."""
        rc = lib.zk_read_view_ranges_dev(self._h, self._ptr(d_comp), comp_size, self._ptr(d_c_off), self._ptr(d_d_off), n_frames,
                                         self._ptr(d_view_ids) if d_view_ids is not None else None, self._ptr(d_view_off), view_count,
                                         self._ptr(d_offs), self._ptr(d_lens), self._ptr(d_dst_off) if d_dst_off is not None else None, count,
                                         self._ptr(d_dst) if d_dst is not None else None, dst_cap, int(verify),
                                         self._ptr(d_status) if d_status is not None else None, stream)
        if rc <= -1000 and rc != -1001:
            self._raise(rc)
        return rc

    def read_ranges(self, comp, c_off, d_off, offs, lens, verify=True, packed=False):
        """Batched reads from host data (zk_read_ranges) -> (list of bytes, one per range -- b"" for a range that failed validation --, int32
        status array).  packed=True: (one bytes object with the ranges back to back, uint64 offsets of count + 1 entries, status array)."""
        comp = np.frombuffer(comp, dtype=np.uint8) if not isinstance(comp, np.ndarray) else comp
        c_off, d_off, offs, lens = _u64(c_off), _u64(d_off), _u64(offs), _u64(lens)
        count = len(offs)
        total = int(d_off[-1])
        ok = [int(o) <= total and int(n) <= total - int(o) for o, n in zip(offs, lens)]
        pk = np.zeros(count + 1, np.uint64)
        pk[1:] = np.cumsum([int(n) if k else 0 for n, k in zip(lens, ok)], dtype=np.uint64)
        out = np.empty(max(int(pk[-1]), 1), np.uint8)
        status = np.zeros(max(count, 1), np.int32)
        rc = lib.zk_read_ranges(self._h, comp.ctypes.data, comp.size, c_off.ctypes.data, d_off.ctypes.data, len(d_off) - 1,
                                offs.ctypes.data, lens.ctypes.data, None, count, out.ctypes.data, int(pk[-1]), int(verify), status.ctypes.data)
        if rc <= -1000 and rc != -1001:
            self._raise(rc)
        if packed:
            return out[:int(pk[-1])].tobytes(), pk, status[:count]
        return [out[int(pk[i]):int(pk[i + 1])].tobytes() for i in range(count)], status[:count]

    def ranges_frames_decoded(self):
        """Frames the last read_ranges* call decoded, every touched frame once (zk_engine_ranges_frames_decoded)."""
        return int(lib.zk_engine_ranges_frames_decoded(self._h))

    def xxh64_frames_dev(self, d_data, d_off, count, d_out, stream=None):
        rc = lib.zk_xxh64_frames_dev(self._h, self._ptr(d_data), self._ptr(d_off), count, self._ptr(d_out), stream)
        if rc != 0:
            self._raise(rc)


class DedupIndex:
    """What an archive already holds, for Engine.dedup_against_dev / encode_dedup_against_dev (zk_dedup_index): the keys and lengths of its
    frames and a table over them, on the device.  It keeps the engine alive; close() it before the engine."""

    def __init__(self, engine):
        h = lib.zk_dedup_index_create(engine._h)
        if not h:
            raise MemoryError("zk_dedup_index_create")
        self._h = C.c_void_p(h)
        self._engine = engine

    @property
    def count(self) -> int:
        return int(lib.zk_dedup_index_count(self._h))

    def __len__(self):
        return self.count

    def _check(self, rc):
        if rc != 0:
            self._engine._raise(rc)

    def add(self, keys, d_sizes):
        """the next len(keys) archive frames, from host arrays: their keys (Engine.frame_keys, or export) and decoded sizes"""
        k = _u64(keys)
        d = np.ascontiguousarray(np.asarray(d_sizes, dtype=np.uint32))
        if len(k) != len(d):
            raise ValueError("keys and d_sizes differ in length")
        self._check(lib.zk_dedup_index_add(self._h, k.ctypes.data, d.ctypes.data, len(k)))

    def add_dev(self, d_keys, d_d_sizes, count, stream=None):
        self._check(lib.zk_dedup_index_add_dev(self._h, Engine._ptr(d_keys), Engine._ptr(d_d_sizes), count, stream))

    def add_archive_dev(self, d_comp, comp_size, d_c_off, d_d_off, n_frames, stream=None):
        """decodes the archive's frames count .. n_frames - 1 on the device, keys them and adds them"""
        self._check(lib.zk_dedup_index_add_archive_dev(self._h, Engine._ptr(d_comp), comp_size, Engine._ptr(d_c_off), Engine._ptr(d_d_off), n_frames, stream))

    def export(self, first=0, count=None):
        """-> (keys np.uint64, d_sizes np.uint32) of frames [first, first + count)"""
        count = self.count - first if count is None else count
        keys, sizes = np.zeros(max(count, 1), np.uint64), np.zeros(max(count, 1), np.uint32)
        self._check(lib.zk_dedup_index_export(self._h, first, count, keys.ctypes.data, sizes.ctypes.data))
        return keys[:count], sizes[:count]

    def truncate(self, count):
        self._check(lib.zk_dedup_index_truncate(self._h, count))

    def compact_dev(self, d_remap, n_frames, stream=None):
        """the index after the removal zk_compact_archive_dev made: d_remap as that call wrote it, n_frames == count"""
        self._check(lib.zk_dedup_index_compact_dev(self._h, Engine._ptr(d_remap), n_frames, stream))

    def close(self):
        if getattr(self, "_h", None):
            if self._engine._h:
                lib.zk_dedup_index_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DedupStore:
    """A growing device-resident archive and its DedupIndex: append() stores the chunks the archive does not hold yet, read() returns any
    list of chunks, read_ranges() byte ranges of a snapshot, compact() drops the chunks no kept snapshot uses.  Python over the device calls only (chunk_boundaries_dev,
    encode_dedup_against_dev, decode_frame_list_dev, read_view_ranges_dev, mark_frames_dev, compact_archive_dev, remap_ids_dev)."""

    def __init__(self, engine, level=1, checksum=True, dictionary=None):
        import torch
        self.engine, self.level, self.checksum, self.dictionary = engine, level, checksum, dictionary
        self.index = DedupIndex(engine)
        self._dev = torch.device("cuda", torch.cuda.current_device())
        self._comp = torch.zeros(1 << 16, dtype=torch.uint8, device=self._dev)
        self.comp_size = 0
        self._c_off = np.zeros(1, np.uint64)
        self._d_off = np.zeros(1, np.uint64)

    @property
    def n_frames(self) -> int:
        return len(self._c_off) - 1

    def _dev_u64(self, a):
        import torch
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64).copy()).to(self._dev)

    def append(self, data, offsets=None, avg_size=0, min_size=0, max_size=0):
        """Stores `data` cut by `offsets` (None: by content, chunk_boundaries_dev with avg_size / min_size / max_size).  Returns (ids, offsets):
        np.uint32 archive frame of every chunk, np.uint64 offsets of the chunks; read(ids, offsets) returns the data."""
        import torch
        data = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else data
        n = len(data)
        d_src = torch.from_numpy(data.copy()).to(self._dev) if n else torch.zeros(1, dtype=torch.uint8, device=self._dev)
        d_off = self.engine.chunk_boundaries_dev(d_src, n, avg_size, min_size, max_size) if offsets is None else self._dev_u64(offsets)
        off = d_off.cpu().numpy().view(np.uint64).copy()
        count = len(off) - 1
        if count <= 0:
            return np.zeros(0, np.uint32), off
        nb = int(off[count] - off[0])
        bound = int(lib.zk_compress_bound_list(nb, count, int(self.dictionary is not None)))
        need = self.comp_size + bound + 64
        if need > self._comp.numel():
            grown = torch.zeros(max(need, 2 * self._comp.numel()), dtype=torch.uint8, device=self._dev)
            grown[:self.comp_size] = self._comp[:self.comp_size]
            self._comp = grown
        ids, fresh, cs, ds = (torch.zeros(count, dtype=torch.int32, device=self._dev) for _ in range(4))
        m = self.n_frames
        torch.cuda.synchronize()
        nf, wr = self.engine.encode_dedup_against_dev(self.index, self._comp, self.comp_size, self._dev_u64(self._c_off), self._dev_u64(self._d_off), m,
                                                      d_src, d_off, count, self.level, self.checksum, self._comp.data_ptr() + self.comp_size, bound, ids,
                                                      fresh, cs, ds, dictionary=self.dictionary)
        self._c_off = np.concatenate([self._c_off, self._c_off[-1] + np.cumsum(cs[:nf].cpu().numpy().view(np.uint32), dtype=np.uint64)])
        self._d_off = np.concatenate([self._d_off, self._d_off[-1] + np.cumsum(ds[:nf].cpu().numpy().view(np.uint32), dtype=np.uint64)])
        self.comp_size += wr
        return ids.cpu().numpy().view(np.uint32).copy(), off

    def read(self, ids, offsets):
        """the bytes of archive frames `ids` laid out by `offsets` (both as append returned them)"""
        import torch
        ids = np.ascontiguousarray(np.asarray(ids, dtype=np.uint32))
        off = _u64(offsets)
        count = len(ids)
        if count == 0:
            return b""
        n = int(off[count] - off[0])
        dst = torch.zeros(n + 64, dtype=torch.uint8, device=self._dev)
        d_ids = torch.from_numpy(ids.view(np.int32).copy()).to(self._dev)
        torch.cuda.synchronize()
        rc = self.engine.decode_frame_list_dev(self._comp, self.comp_size, self._dev_u64(self._c_off), self._dev_u64(self._d_off), d_ids,
                                               self._dev_u64(off - off[0]), count, dst, n, True)
        if rc != 0:
            self.engine._raise(rc)
        return dst[:n].cpu().numpy().tobytes()

    def read_ranges(self, ids, offsets, offs, lens):
        """Byte ranges of a snapshot (ids, offsets as append returned them): [offs[i], offs[i] + lens[i]) in the coordinates of `offsets` -> a
        list of bytes.  Only the chunks the ranges touch are decoded, each archive frame once (read_view_ranges_dev).  A range outside the
        snapshot or a chunk that does not decode raises."""
        import torch
        ids = np.ascontiguousarray(np.asarray(ids, dtype=np.uint32))
        off, offs, lens = _u64(offsets), _u64(offs), _u64(lens)
        count = len(offs)
        if count == 0:
            return []
        if len(off) != len(ids) + 1:
            raise ValueError("offsets must have one entry more than ids")
        at = np.zeros(count + 1, np.uint64)
        at[1:] = np.cumsum(lens, dtype=np.uint64)
        n = int(at[count])
        dst = torch.zeros(n + 64, dtype=torch.uint8, device=self._dev)
        d_ids = torch.from_numpy(ids.view(np.int32).copy()).to(self._dev) if len(ids) else None
        torch.cuda.synchronize()
        rc = self.engine.read_view_ranges_dev(self._comp, self.comp_size, self._dev_u64(self._c_off), self._dev_u64(self._d_off), self.n_frames, d_ids,
                                              self._dev_u64(off), len(ids), self._dev_u64(offs), self._dev_u64(lens), self._dev_u64(at[:count]), count, dst, n, True)
        if rc != 0:
            self.engine._raise(rc)
        out = dst[:n].cpu().numpy()
        return [out[int(at[i]):int(at[i + 1])].tobytes() for i in range(count)]

    def digests(self, first=0, count=None, algo="sha256"):
        """the digests of the stored chunks [first, first + count) (count None: to the end), of their decoded content -> np.uint8[count, 32]
        (archive_digests_dev over the store's own buffers).  A chunk that does not decode raises."""
        import torch
        count = self.n_frames - first if count is None else count
        if first < 0 or count < 0 or first + count > self.n_frames:
            raise ValueError("chunks [%d, %d) are not in a store of %d" % (first, first + count, self.n_frames))
        if count == 0:
            return np.zeros((0, 32), np.uint8)
        out = torch.zeros(count * 32, dtype=torch.uint8, device=self._dev)
        torch.cuda.synchronize()
        rc = self.engine.archive_digests_dev(self._comp, self.comp_size, self._dev_u64(self._c_off), self._dev_u64(self._d_off), first, count, out, algo)
        if rc != 0:
            self.engine._raise(rc)
        return out.cpu().numpy().reshape(count, 32)

    def compact(self, keep):
        """Drops every chunk that none of the snapshots in `keep` (a list of `ids` arrays, as append returned them) uses: the archive is
        compacted in place, the index with it.  Returns the renumbered ids arrays in the same order; read() with them returns what it
        returned before."""
        import torch
        n = self.n_frames
        keep = [np.ascontiguousarray(np.asarray(k, dtype=np.uint32)) for k in keep]
        if n == 0:
            return keep
        live = torch.zeros(n, dtype=torch.uint8, device=self._dev)
        d_keep = [torch.from_numpy(k.view(np.int32).copy()).to(self._dev) for k in keep]
        d_c, d_d = self._dev_u64(self._c_off), self._dev_u64(self._d_off)
        remap = torch.zeros(n, dtype=torch.int32, device=self._dev)
        torch.cuda.synchronize()
        for k, d in zip(keep, d_keep):
            if len(k):
                self.engine.mark_frames_dev(d, len(k), n, live)
        nk, wr = self.engine.compact_archive_dev(self._comp, self.comp_size, d_c, d_d, n, live, self._comp, self._comp.numel(), d_c, d_d, remap)
        for k, d in zip(keep, d_keep):
            if len(k):
                self.engine.remap_ids_dev(remap, n, d, len(k))
        self.index.compact_dev(remap, n)
        self._c_off = d_c[:nk + 1].cpu().numpy().view(np.uint64).copy()
        self._d_off = d_d[:nk + 1].cpu().numpy().view(np.uint64).copy()
        self.comp_size = wr
        return [d.cpu().numpy().view(np.uint32).copy() for d in d_keep]

    def close(self):
        self.index.close()
