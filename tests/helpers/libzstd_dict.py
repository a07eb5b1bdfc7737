"""TEST INFRASTRUCTURE -- the real libzstd 1.5.7 as the judge of dictionaries and of frames written against them (oracle/libzstd_ref.py
finds the library; tests/test_dict.py loads it the same way): ZSTD_decompress_usingDict for a (dictionary, frame) pair,
ZSTD_DCtx_loadDictionary for a dictionary alone.  Nothing of the product imports this."""
import ctypes as C

from oracle import libzstd_ref


class Judge:
    def __init__(self, z):
        self.z = z
        z.ZSTD_decompress_usingDict.restype = C.c_size_t
        z.ZSTD_decompress_usingDict.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]
        z.ZSTD_DCtx_loadDictionary.restype = C.c_size_t
        z.ZSTD_DCtx_loadDictionary.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        z.ZSTD_getErrorCode.restype = C.c_int
        z.ZSTD_getErrorCode.argtypes = [C.c_size_t]
        self.dctx = z.ZSTD_createDCtx()

    def using_dict(self, frame, cap, dictionary):
        """-> the decoded bytes, or the negated ZSTD_ErrorCode"""
        frame, dictionary = bytes(frame), bytes(dictionary) if dictionary else None
        out = C.create_string_buffer(max(cap, 1))
        n = self.z.ZSTD_decompress_usingDict(self.dctx, out, cap, frame, len(frame), dictionary, len(dictionary) if dictionary else 0)
        return -self.z.ZSTD_getErrorCode(n) if self.z.ZSTD_isError(n) else out.raw[:n]

    def load_dictionary(self, dictionary):
        """-> 0, or the ZSTD_ErrorCode ZSTD_DCtx_loadDictionary gives (a fresh context: nothing of an earlier load stays)"""
        dictionary = bytes(dictionary)
        dctx = self.z.ZSTD_createDCtx()
        n = self.z.ZSTD_DCtx_loadDictionary(dctx, dictionary, len(dictionary))
        self.z.ZSTD_freeDCtx(dctx)
        return self.z.ZSTD_getErrorCode(n) if self.z.ZSTD_isError(n) else 0

    def close(self):
        self.z.ZSTD_freeDCtx(self.dctx)


def judge():
    """the judge, or None where libzstd 1.5.7 is not in the image (tests/test_dict.py skips there too)"""
    z = libzstd_ref.load("1.5.7")
    return Judge(z) if z is not None else None
