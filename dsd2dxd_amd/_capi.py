"""ctypes binding of include/dsd2dxd_amd.h (the same calls the Rust `extern "C"` block in
INTEGRATION.md makes).  Loading fails loudly when the HIP library has not been built."""
import ctypes as C
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
KERNEL_AUTO, KERNEL_LUT, KERNEL_MFMA = 0, 1, 2
# d2d_params.filter (D2D_FILTER_*): the reference CLI's letters, and "S", the equiripple filter of the 48 kHz multiples in two stages
FILTER_EQUIRIPPLE, FILTER_XLD, FILTER_DSD2PCM, FILTER_CHEBYSHEV, FILTER_EQUIRIPPLE_CASCADE = "E", "X", "D", "C", "S"
# d2d_params.debug_flags (include/dsd2dxd_amd.h: D2D_DBG_*): diagnostic dispatch switches, 0 in production
DBG_NO_MX, DBG_NO_GAINQ, DBG_NO_COOP, DBG_HOST_STAGED, DBG_NO_PIPE, DBG_MFMA_V1, DBG_NO_INTQ, DBG_NS_GENERAL = (1 << i for i in range(8))
DBG_TAPS32_2PASS = 1 << 16
DBG_NO_DITHER_TABLE = 1 << 17
# files a call needs at one output index before it hashes its dither words into a table (d2d_engine.cpp: kDitherTableMinFiles)
DITHER_TABLE_MIN_FILES = 48


def dbg_waves(n):
    """debug_flags bits 8..15: waves per block of the matrix-core kernels"""
    return (int(n) & 0xFF) << 8



def library_path():
    # D2D_AMD_LIB: development A/B builds of the same library (tools/ab_build.sh); never a different implementation
    return os.environ.get("D2D_AMD_LIB") or os.path.join(HERE, "libdsd2dxd_amd.so")


def build_library(force=False):
    """hipcc --offload-arch=gfx950 build of csrc/ (cross-compiles without a GPU)."""
    args = ["make", "-C", os.path.join(HERE, "csrc"), "-j4"]
    if force:
        subprocess.check_call(args + ["clean"])
    subprocess.check_call(args)
    return library_path()


class Params(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("dsd_rate", C.c_uint32), ("output_rate", C.c_uint32),
                ("channels", C.c_uint32), ("fmt", C.c_uint32), ("endianness", C.c_uint32),
                ("block_size", C.c_uint32), ("filter", C.c_uint32), ("bit_depth", C.c_uint32),
                ("dither", C.c_uint32), ("kernel", C.c_uint32), ("device", C.c_int32),
                ("level_db", C.c_double), ("seed", C.c_uint64),
                ("channel_first", C.c_uint32), ("channel_count", C.c_uint32),
                ("tap_bits", C.c_uint32), ("debug_flags", C.c_uint32)]


class FileIO(C.Structure):
    _fields_ = [("dsd", C.c_void_p), ("bytes_per_channel", C.c_size_t), ("pcm", C.c_void_p),
                ("pcm_capacity_bytes", C.c_size_t), ("frames_out", C.c_size_t)]


class Info(C.Structure):
    _fields_ = [("decimation", C.c_uint32), ("ntaps", C.c_uint32), ("scale_bits", C.c_uint32),
                ("resamp_L", C.c_uint32), ("resamp_M", C.c_uint32), ("resamp_P", C.c_uint32),
                ("kernel", C.c_uint32), ("abi_version", C.c_uint32), ("filter_name", C.c_char * 32)]


class FlacResult(C.Structure):
    _fields_ = [("bytes_out", C.c_uint64), ("min_frame_bytes", C.c_uint32), ("max_frame_bytes", C.c_uint32)]


class FlacIO(C.Structure):
    """d2d_flac_io: one file of a d2d_flac_encode_device call (DEVICE pointers; `result` device or pinned host)"""
    _fields_ = [("pcm", C.c_void_p), ("frames", C.c_size_t), ("first_block", C.c_uint32), ("final", C.c_int32),
                ("out", C.c_void_p), ("out_capacity_bytes", C.c_size_t), ("result", C.c_void_p),
                ("blocks", C.c_size_t), ("frames_consumed", C.c_size_t)]


class FlacStreamStats(C.Structure):
    _fields_ = [("samples_per_channel", C.c_uint64), ("blocks", C.c_uint64),
                ("min_frame_bytes", C.c_uint32), ("max_frame_bytes", C.c_uint32)]


class FlacCheck(C.Structure):
    """d2d_flac_check: what a verify or decode call found"""
    _fields_ = [("samples_checked", C.c_uint64), ("blocks_checked", C.c_uint32), ("bad_blocks", C.c_uint32),
                ("first_bad_block", C.c_uint32), ("first_bad_reason", C.c_uint32)]

    def as_tuple(self):
        return (self.samples_checked, self.blocks_checked, self.bad_blocks, self.first_bad_block, self.first_bad_reason)


class FlacVerifyStats(C.Structure):
    """d2d_flac_verify_stats: the blocks the cooperative path accepted, and those the serial parser decided"""
    _fields_ = [("fast_blocks", C.c_uint32), ("fallback_blocks", C.c_uint32)]

    def as_tuple(self):
        return (self.fast_blocks, self.fallback_blocks)


class FlacMd5State(C.Structure):
    """d2d_flac_md5_state: one file's MD5 so far, 96 bytes (public layout: a caller may keep, copy or build one)"""
    _fields_ = [("h", C.c_uint32 * 4), ("bytes", C.c_uint64), ("tail_bytes", C.c_uint32), ("reserved", C.c_uint32),
                ("tail", C.c_uint8 * 64)]


class FlacMd5IO(C.Structure):
    """d2d_flac_md5_io: one file of a d2d_flac_md5_update_device call (DEVICE pointer, 16-byte aligned)"""
    _fields_ = [("pcm", C.c_void_p), ("frames", C.c_size_t)]


class LoudCell(C.Structure):
    """d2d_loud_cell: (energy, peak) of one sub-block (100 ms) of one channel"""
    _fields_ = [("energy", C.c_double), ("peak", C.c_double)]


class LoudIO(C.Structure):
    """d2d_loud_io: one file of a d2d_loud_measure_device / _host call; subblocks, cells_out and next_subblock are written at return"""
    _fields_ = [("pcm", C.c_void_p), ("frames", C.c_size_t), ("first_frame", C.c_uint64), ("first_subblock", C.c_uint64),
                ("final", C.c_int32), ("reserved", C.c_uint32), ("cells", C.c_void_p), ("cells_capacity", C.c_size_t),
                ("subblocks", C.c_size_t), ("cells_out", C.c_size_t), ("next_subblock", C.c_uint64)]


class TruePeakIO(C.Structure):
    """d2d_tpeak_io: one file of a d2d_true_peak_measure_device / _host call; subblocks, peaks_out and next_subblock are written at return"""
    _fields_ = [("pcm", C.c_void_p), ("frames", C.c_size_t), ("first_frame", C.c_uint64), ("first_subblock", C.c_uint64),
                ("final", C.c_int32), ("reserved", C.c_uint32), ("peaks", C.c_void_p), ("peaks_capacity", C.c_size_t),
                ("subblocks", C.c_size_t), ("peaks_out", C.c_size_t), ("next_subblock", C.c_uint64)]


class LoudResult(C.Structure):
    """d2d_loud_result: integrated loudness, sample peak and the ReplayGain track gain of one stream"""
    _fields_ = [("lufs", C.c_double), ("peak", C.c_double), ("gain_db", C.c_double), ("valid", C.c_int32), ("reserved", C.c_uint32),
                ("blocks_total", C.c_uint64), ("blocks_gated", C.c_uint64)]


class Mix(C.Structure):
    """d2d_mix: out_channels rows x channels columns of Q15 coefficients (d2d_create_mix, d2d_mix_frames_host)"""
    _fields_ = [("struct_size", C.c_uint32), ("out_channels", C.c_uint32), ("coef", C.POINTER(C.c_int32))]


MIX_UNITY = 32768                                                       # a Q15 gain of 1.0
# D2D_MIX_LAYOUT_*
MIX_LAYOUT_AUTO, MIX_LAYOUT_STEREO, MIX_LAYOUT_LRC, MIX_LAYOUT_QUAD, MIX_LAYOUT_5_0, MIX_LAYOUT_5_1, MIX_LAYOUT_LRC_LFE = 0, 2, 3, 4, 5, 6, 7


class Segment(C.Structure):
    """d2d_segment: `bytes` bytes from src to dst (d2d_segments_move_device / _host)"""
    _fields_ = [("dst", C.c_void_p), ("src", C.c_void_p), ("bytes", C.c_size_t)]


class PackSrc(C.Structure):
    """d2d_pack_src: one source of d2d_segments_pack_device / _host; `bytes` points at the uint64 length, read where the call runs"""
    _fields_ = [("base", C.c_void_p), ("bytes", C.c_void_p), ("max_bytes", C.c_size_t)]


FLAC_VERIFY_AUTO, FLAC_VERIFY_SERIAL, FLAC_VERIFY_COOP = 0, 1, 2       # D2D_FLAC_VERIFY_*
# D2D_FLAC_BAD_*
(FLAC_BAD_NONE, FLAC_BAD_SIZE, FLAC_BAD_HEADER, FLAC_BAD_CRC8, FLAC_BAD_CRC16, FLAC_BAD_UNSUPPORTED, FLAC_BAD_SYNTAX, FLAC_BAD_LENGTH,
 FLAC_BAD_SAMPLES) = range(9)
FLAC_NO_BAD_BLOCK = 0xFFFFFFFF
ERR_VERIFY = -60

FLAC_BLOCK = 4096
FLAC_EFFORT_FIXED2, FLAC_EFFORT_SEARCH, FLAC_EFFORT_LPC = 0, 1, 12      # D2D_FLAC_EFFORT_*

READ_FN = C.CFUNCTYPE(C.c_long, C.c_void_p, C.POINTER(C.c_uint8), C.c_size_t)
WRITE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t)
PROGRESS_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_float)

STREAMS_VERIFY, STREAMS_MD5 = 1, 2                                      # D2D_STREAMS_*
PACK_GAVE_UP = 0xFFFFFFFFFFFFFFFF                                       # every entry of a pack's table when a length was above its maximum


class StreamIO(C.Structure):
    """d2d_stream_io: one file of d2d_convert_streams_flac; stats, check and md5 are written by the call"""
    _fields_ = [("read", READ_FN), ("read_user", C.c_void_p), ("write", WRITE_FN), ("write_user", C.c_void_p),
                ("total_bytes_per_channel", C.c_uint64), ("loud", C.c_void_p), ("stats", FlacStreamStats), ("check", FlacCheck),
                ("md5", C.c_uint8 * 16)]


class StreamsOptions(C.Structure):
    """d2d_streams_options"""
    _fields_ = [("struct_size", C.c_uint32), ("bit_depth", C.c_uint32), ("effort", C.c_uint32), ("flags", C.c_uint32),
                ("chunk_bytes_per_channel", C.c_size_t), ("cancel", C.POINTER(C.c_int)), ("progress", PROGRESS_FN),
                ("progress_user", C.c_void_p), ("device_calls", C.POINTER(C.c_uint64)), ("chunks", C.POINTER(C.c_uint64))]


EXPORTS = ["d2d_create", "d2d_create_error", "d2d_destroy", "d2d_reset", "d2d_last_error",
           "d2d_frame_bytes", "d2d_next_frames", "d2d_translate", "d2d_translate_batch_device",
           "d2d_translate_batch_host",
           "d2d_peak", "d2d_peak_dbfs", "d2d_convert_stream", "d2d_tables_bytes",
           "d2d_tables_export_device", "d2d_tables_import_device", "d2d_get_info", "d2d_kernel_name",
           "d2d_profile_enable", "d2d_profile_read", "d2d_profile_read_all",
           "d2d_seek", "d2d_tell", "d2d_preroll_bytes", "d2d_slice_align_bytes", "d2d_prime", "d2d_prime_batch_device",
           "d2d_flac_bound_bytes", "d2d_flac_workspace_bytes", "d2d_flac_encode_device", "d2d_flac_error",
           "d2d_flac_encode_host", "d2d_convert_stream_flac",
           "d2d_flac_encode_device_effort", "d2d_flac_encode_host_effort", "d2d_convert_stream_flac_effort",
           "d2d_flac_verify_device", "d2d_flac_verify_host", "d2d_flac_decode_host", "d2d_convert_stream_flac_verified",
           "d2d_flac_verify_device_method", "d2d_flac_verify_host_method",
           "d2d_flac_md5_init_host", "d2d_flac_md5_init_device", "d2d_flac_md5_update_device", "d2d_flac_md5_final_device",
           "d2d_flac_md5_update_host", "d2d_flac_md5_final_host", "d2d_convert_stream_flac_md5",
           "d2d_loud_coefficients", "d2d_loud_measure_device", "d2d_loud_measure_host", "d2d_loud_create", "d2d_loud_add",
           "d2d_loud_finish", "d2d_loud_destroy", "d2d_convert_stream_flac_loud",
           "d2d_true_peak_measure_device", "d2d_true_peak_measure_host", "d2d_loud_set_true_peak", "d2d_loud_add_true_peaks",
           "d2d_loud_true_peak", "d2d_dither_table_calls",
           "d2d_segments_move_device", "d2d_segments_move_host", "d2d_segments_pack_device", "d2d_segments_pack_host",
           "d2d_convert_streams_flac", "d2d_loud_finish_album", "d2d_loud_true_peak_album",
           "d2d_create_mix", "d2d_get_mix", "d2d_input_channels", "d2d_mix_preset", "d2d_mix_frames_host", "d2d_mix_error",
           "d2d_create_half", "d2d_half_factor", "d2d_half_taps", "d2d_half_frames_host", "d2d_half_frames_device", "d2d_half_error"]

_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    path = library_path()
    if not os.path.exists(path):
        raise RuntimeError(f"{path} is missing: build the HIP extension first "
                           "(python -c 'import __graft_entry__ as g; g.build()'). There is no fallback path.")
    # torch ships its own libamdhip64.so.7 / libhsa-runtime64.so.1 and asks for them by file name, so
    # it does not reuse an already-loaded /opt/rocm copy; two HIP runtimes in one process leave the
    # second without a GPU.  Loading torch FIRST makes the loader satisfy this library's
    # DT_NEEDED libamdhip64.so.7 with torch's copy (same soname): one runtime, shared device pointers.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(path)
    L.d2d_create.argtypes = [C.POINTER(Params), C.c_uint32, C.POINTER(C.c_void_p)]
    L.d2d_create.restype = C.c_int
    L.d2d_create_error.restype = C.c_char_p
    L.d2d_destroy.argtypes = [C.c_void_p]
    L.d2d_destroy.restype = None
    L.d2d_reset.argtypes = [C.c_void_p]
    L.d2d_last_error.argtypes = [C.c_void_p]
    L.d2d_last_error.restype = C.c_char_p
    L.d2d_frame_bytes.argtypes = [C.c_void_p]
    L.d2d_frame_bytes.restype = C.c_size_t
    L.d2d_next_frames.argtypes = [C.c_void_p, C.c_uint32, C.c_size_t]
    L.d2d_next_frames.restype = C.c_size_t
    L.d2d_translate.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.d2d_translate_batch_device.argtypes = [C.c_void_p, C.POINTER(FileIO), C.c_uint32, C.c_void_p]
    L.d2d_translate_batch_host.argtypes = [C.c_void_p, C.POINTER(FileIO), C.c_uint32, C.c_size_t]
    L.d2d_translate_batch_host.restype = C.c_int
    L.d2d_peak.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_double)]
    L.d2d_peak_dbfs.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_float)]
    L.d2d_convert_stream.argtypes = [C.c_void_p, READ_FN, C.c_void_p, WRITE_FN, C.c_void_p,
                                     C.POINTER(C.c_int), PROGRESS_FN, C.c_void_p, C.c_uint64, C.c_size_t]
    L.d2d_tables_bytes.argtypes = [C.c_void_p]
    L.d2d_tables_bytes.restype = C.c_size_t
    L.d2d_tables_export_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    L.d2d_tables_import_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    L.d2d_get_info.argtypes = [C.c_void_p, C.POINTER(Info)]
    L.d2d_kernel_name.argtypes = [C.c_void_p]
    L.d2d_kernel_name.restype = C.c_char_p
    if hasattr(L, "d2d_dither_table_calls"):      # (a D2D_AMD_LIB build of an older tree lacks it; the shipped library is held to EXPORTS by the tests)
        L.d2d_dither_table_calls.argtypes = [C.c_void_p]
        L.d2d_dither_table_calls.restype = C.c_uint64
    L.d2d_profile_enable.argtypes = [C.c_void_p, C.c_int]
    L.d2d_profile_read.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
    L.d2d_profile_read_all.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
    L.d2d_seek.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64]
    L.d2d_tell.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.d2d_preroll_bytes.argtypes = [C.c_void_p]
    L.d2d_preroll_bytes.restype = C.c_size_t
    L.d2d_slice_align_bytes.argtypes = [C.c_void_p]
    L.d2d_slice_align_bytes.restype = C.c_size_t
    L.d2d_prime.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    L.d2d_prime_batch_device.argtypes = [C.c_void_p, C.POINTER(FileIO), C.c_uint32, C.c_void_p]
    L.d2d_flac_bound_bytes.argtypes = [C.c_uint32, C.c_uint32, C.c_size_t, C.c_int]
    L.d2d_flac_bound_bytes.restype = C.c_size_t
    L.d2d_flac_workspace_bytes.argtypes = [C.c_uint32, C.c_uint32, C.c_size_t, C.c_int]
    L.d2d_flac_workspace_bytes.restype = C.c_size_t
    L.d2d_flac_encode_device.argtypes = [C.c_uint32, C.c_uint32, C.POINTER(FlacIO), C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p]
    L.d2d_flac_error.restype = C.c_char_p
    L.d2d_flac_encode_host.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t, C.c_uint32, C.c_int, C.c_void_p, C.c_size_t,
                                       C.POINTER(FlacResult), C.POINTER(C.c_size_t)]
    L.d2d_convert_stream_flac.argtypes = [C.c_void_p, C.c_uint32, READ_FN, C.c_void_p, WRITE_FN, C.c_void_p, C.POINTER(C.c_int),
                                          PROGRESS_FN, C.c_void_p, C.c_uint64, C.c_size_t, C.POINTER(FlacStreamStats)]
    L.d2d_flac_encode_device_effort.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(FlacIO), C.c_uint32, C.c_void_p, C.c_size_t,
                                                C.c_void_p]
    L.d2d_flac_encode_host_effort.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t, C.c_uint32, C.c_int, C.c_void_p,
                                              C.c_size_t, C.POINTER(FlacResult), C.POINTER(C.c_size_t)]
    L.d2d_convert_stream_flac_effort.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, READ_FN, C.c_void_p, WRITE_FN, C.c_void_p,
                                                 C.POINTER(C.c_int), PROGRESS_FN, C.c_void_p, C.c_uint64, C.c_size_t,
                                                 C.POINTER(FlacStreamStats)]
    L.d2d_flac_verify_device.argtypes = [C.c_uint32, C.c_uint32, C.POINTER(FlacIO), C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    L.d2d_flac_verify_host.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t, C.c_uint32, C.c_int, C.c_void_p, C.c_size_t,
                                       C.c_void_p, C.POINTER(FlacCheck)]
    L.d2d_flac_verify_device_method.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(FlacIO), C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p,
                                                C.c_void_p, C.c_void_p]
    L.d2d_flac_verify_host_method.argtypes = L.d2d_flac_verify_host.argtypes + [C.c_uint32, C.POINTER(FlacVerifyStats)]
    L.d2d_flac_decode_host.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p, C.c_size_t,
                                       C.POINTER(C.c_size_t), C.POINTER(FlacCheck)]
    L.d2d_convert_stream_flac_verified.argtypes = L.d2d_convert_stream_flac_effort.argtypes + [C.POINTER(FlacCheck)]
    L.d2d_flac_md5_init_host.argtypes = [C.POINTER(FlacMd5State), C.c_uint32]
    L.d2d_flac_md5_init_host.restype = None
    L.d2d_flac_md5_init_device.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
    L.d2d_flac_md5_update_device.argtypes = [C.c_uint32, C.c_uint32, C.POINTER(FlacMd5IO), C.c_uint32, C.c_void_p, C.c_void_p]
    L.d2d_flac_md5_final_device.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    L.d2d_flac_md5_update_host.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t, C.POINTER(FlacMd5State)]
    L.d2d_flac_md5_final_host.argtypes = [C.POINTER(FlacMd5State), C.c_void_p]
    L.d2d_convert_stream_flac_md5.argtypes = L.d2d_convert_stream_flac_verified.argtypes + [C.c_void_p]
    L.d2d_loud_coefficients.argtypes = [C.c_uint32, C.POINTER(C.c_double)]
    L.d2d_loud_measure_device.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(LoudIO), C.c_uint32, C.c_void_p]
    L.d2d_loud_measure_host.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(LoudIO)]
    L.d2d_loud_create.argtypes = [C.c_uint32, C.c_uint32, C.POINTER(C.c_double), C.POINTER(C.c_void_p)]
    L.d2d_loud_add.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    L.d2d_loud_finish.argtypes = [C.c_void_p, C.POINTER(LoudResult)]
    L.d2d_loud_destroy.argtypes = [C.c_void_p]
    L.d2d_loud_destroy.restype = None
    L.d2d_convert_stream_flac_loud.argtypes = L.d2d_convert_stream_flac_md5.argtypes + [C.c_void_p]
    L.d2d_true_peak_measure_device.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(TruePeakIO), C.c_uint32, C.c_void_p]
    L.d2d_true_peak_measure_host.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(TruePeakIO)]
    L.d2d_loud_set_true_peak.argtypes = [C.c_void_p, C.c_int]
    L.d2d_loud_add_true_peaks.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    L.d2d_loud_true_peak.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
    if hasattr(L, "d2d_segments_move_device"):    # (as above: a D2D_AMD_LIB build of an older tree lacks the album calls)
        L.d2d_segments_move_device.argtypes = [C.POINTER(Segment), C.c_uint32, C.c_void_p]
        L.d2d_segments_move_host.argtypes = [C.POINTER(Segment), C.c_uint32]
        L.d2d_segments_pack_device.argtypes = [C.POINTER(PackSrc), C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        L.d2d_segments_pack_host.argtypes = [C.POINTER(PackSrc), C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p]
        L.d2d_convert_streams_flac.argtypes = [C.c_void_p, C.POINTER(StreamIO), C.c_uint32, C.POINTER(StreamsOptions)]
        L.d2d_loud_finish_album.argtypes = [C.POINTER(C.c_void_p), C.c_uint32, C.POINTER(LoudResult)]
        L.d2d_loud_true_peak_album.argtypes = [C.POINTER(C.c_void_p), C.c_uint32, C.POINTER(C.c_double)]
    if hasattr(L, "d2d_create_mix"):              # (as above: a D2D_AMD_LIB build of an older tree lacks the channel matrix)
        L.d2d_create_mix.argtypes = [C.POINTER(Params), C.POINTER(Mix), C.c_uint32, C.POINTER(C.c_void_p)]
        L.d2d_get_mix.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_int32), C.c_size_t]
        L.d2d_input_channels.argtypes = [C.c_void_p]
        L.d2d_input_channels.restype = C.c_uint32
        L.d2d_mix_preset.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_int32), C.POINTER(C.c_uint32)]
        L.d2d_mix_frames_host.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_uint32, C.c_int32, C.POINTER(Mix), C.c_uint32, C.c_uint32,
                                          C.c_double, C.c_uint64, C.c_uint64, C.c_void_p, C.c_size_t, C.c_void_p]
        L.d2d_mix_error.restype = C.c_char_p
    if hasattr(L, "d2d_create_half"):             # (as above: an older tree's build lacks the halved engine)
        L.d2d_create_half.argtypes = [C.POINTER(Params), C.c_uint32, C.POINTER(C.c_void_p)]
        L.d2d_half_factor.argtypes = [C.c_void_p]
        L.d2d_half_factor.restype = C.c_uint32
        L.d2d_half_taps.argtypes = [C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_int32), C.c_size_t]
        L.d2d_half_frames_host.argtypes = [C.POINTER(HalfJob), C.c_uint32, C.c_uint32, C.c_int32, C.c_uint32, C.c_uint32, C.c_double, C.c_uint64]
        L.d2d_half_frames_device.argtypes = L.d2d_half_frames_host.argtypes + [C.c_void_p]
        L.d2d_half_error.restype = C.c_char_p
    _lib = L
    return L


def _mix_struct(coef, channels):
    """(Mix, the int32 array it points at) of a rows x channels table of Q15 integers"""
    import numpy as np
    a = np.ascontiguousarray(np.asarray(coef, dtype=np.int64).reshape(-1, channels) if channels else np.zeros((0, 0)), dtype=np.int32)
    return Mix(C.sizeof(Mix), a.shape[0], a.ctypes.data_as(C.POINTER(C.c_int32))), a


def mix_preset(in_channels, target, layout=MIX_LAYOUT_AUTO):
    """d2d_mix_preset: the fold-down rows of a layout as a list of rows of Q15 integers (target 2: Lo, Ro; 1: mono)"""
    coef, rows = (C.c_int32 * (2 * max(in_channels, 1)))(), C.c_uint32()
    rc = lib().d2d_mix_preset(in_channels, layout, target, coef, C.byref(rows))
    if rc:
        raise D2DError(rc, lib().d2d_mix_error().decode())
    return [list(coef[r * in_channels:(r + 1) * in_channels]) for r in range(rows.value)]


def mix_frames_host(sums, scale_bits, coef, bit_depth=24, dither="X", level_db=0.0, seed=0, first_index=0, capacity=None):
    """d2d_mix_frames_host, the CPU twin of the mix pass: sums an int32 array (channels, frames) of exact FIR sums at scale 2^-scale_bits,
    coef rows x channels Q15 integers.  Returns (frame bytes as a uint8 array, peaks per output channel).  No device."""
    import numpy as np
    x = np.ascontiguousarray(sums, dtype=np.int32)
    channels, frames = x.shape
    m, keep = _mix_struct(coef, channels)
    fb = m.out_channels * (2 if bit_depth == 16 else 4 if bit_depth == 32 else 3)
    cap = frames * fb if capacity is None else capacity
    out = np.zeros(max(cap, 1), dtype=np.uint8)
    peaks = np.zeros(max(m.out_channels, 1), dtype=np.float64)
    rc = lib().d2d_mix_frames_host(x.ctypes.data, frames, frames, channels, scale_bits, C.byref(m), bit_depth, ord(dither.upper()), level_db,
                                   seed, first_index, out.ctypes.data, cap, peaks.ctypes.data)
    if rc:
        raise D2DError(rc, lib().d2d_mix_error().decode())
    return out[:frames * fb], peaks[:m.out_channels]


class HalfJob(C.Structure):
    """d2d_half_job: one file of a call of the 2:1 decimator on its own (d2d_half_frames_host / _device)"""
    _fields_ = [("sums", C.c_void_p), ("stride", C.c_size_t), ("n", C.c_size_t), ("first_index", C.c_uint64),
                ("pcm", C.c_void_p), ("pcm_capacity_bytes", C.c_size_t), ("peaks", C.c_void_p), ("frames_out", C.c_size_t)]


def half_taps():
    """d2d_half_taps: (the decimator's taps as a list of integers, T): h[j] = q[j] * 2^-T"""
    nt, t = C.c_uint32(), C.c_uint32()
    rc = lib().d2d_half_taps(C.byref(nt), C.byref(t), None, 0)
    if not rc:
        taps = (C.c_int32 * nt.value)()
        rc = lib().d2d_half_taps(C.byref(nt), C.byref(t), taps, nt.value)
    if rc:
        raise D2DError(rc, lib().d2d_half_error().decode())
    return list(taps), t.value


def _sample_bytes(bit_depth):
    return 2 if bit_depth == 16 else 4 if bit_depth == 32 else 3


def half_frames_host(lines, first_index, scale_bits, bit_depth=24, dither="X", level_db=0.0, seed=0, capacity=None):
    """d2d_half_frames_host, the CPU twin of the half pass.  lines: one int32 array (channels, NT - 1 + n) per file -- the carried sums, then
    the n new ones; first_index: one absolute index of the first new sum per file.  Returns [(frame bytes as a uint8 array, peaks per channel)]
    per file.  capacity: bytes of every file's buffer (default: what its frames need).  No device."""
    import numpy as np
    nt = len(half_taps()[0])
    xs = [np.ascontiguousarray(x, dtype=np.int32) for x in lines]
    channels = xs[0].shape[0]
    fb = channels * _sample_bytes(bit_depth)
    jobs = (HalfJob * len(xs))()
    outs, peaks = [], []
    for j, x, first in zip(jobs, xs, first_index):
        n = x.shape[1] - (nt - 1)
        frames = ((first + n + 1) >> 1) - ((first + 1) >> 1)
        cap = frames * fb if capacity is None else capacity
        outs.append(np.zeros(max(cap, 1), dtype=np.uint8))
        peaks.append(np.zeros(channels, dtype=np.float64))
        j.sums, j.stride, j.n, j.first_index = x.ctypes.data, x.shape[1], n, first
        j.pcm, j.pcm_capacity_bytes, j.peaks = outs[-1].ctypes.data, cap, peaks[-1].ctypes.data
    rc = lib().d2d_half_frames_host(jobs, len(xs), channels, scale_bits, bit_depth, ord(dither.upper()), level_db, seed)
    if rc:
        raise D2DError(rc, lib().d2d_half_error().decode())
    return [(o[:j.frames_out * fb], p) for o, p, j in zip(outs, peaks, jobs)]


def half_frames_device(jobs, channels, scale_bits, bit_depth=24, dither="X", level_db=0.0, seed=0, stream=None):
    """d2d_half_frames_device: jobs a ctypes array of HalfJob with GPU-addressable sums, pcm and peaks; one launch on `stream`
    (hipStream_t int), returns once it has finished; every frames_out is filled."""
    rc = lib().d2d_half_frames_device(jobs, len(jobs), channels, scale_bits, bit_depth, ord(dither.upper()), level_db, seed, C.c_void_p(stream or 0))
    if rc:
        raise D2DError(rc, lib().d2d_half_error().decode())


def _flac_check(rc):
    if rc:
        raise D2DError(rc, lib().d2d_flac_error().decode())


def flac_bound_bytes(channels, bit_depth, frames, final):
    return lib().d2d_flac_bound_bytes(channels, bit_depth, frames, int(bool(final)))


def flac_workspace_bytes(channels, bit_depth, frames, final):
    return lib().d2d_flac_workspace_bytes(channels, bit_depth, frames, int(bool(final)))


def flac_encode_host(channels, bit_depth, pcm, first_block=0, final=True, capacity=None, effort=0):
    """d2d_flac_encode_host_effort on a bytes-like of interleaved little-endian frames: the sink's own encoder, no device.
    Returns (frame bytes, FlacResult, frames_consumed)."""
    import numpy as np
    buf = np.ascontiguousarray(np.frombuffer(pcm, dtype=np.uint8) if not isinstance(pcm, np.ndarray) else pcm.view(np.uint8).reshape(-1))
    fb = channels * (2 if bit_depth == 16 else 3)
    frames = buf.size // fb if fb else 0
    cap = flac_bound_bytes(channels, bit_depth, frames, final) if capacity is None else capacity
    out = np.zeros(max(cap, 1), dtype=np.uint8)
    res, used = FlacResult(), C.c_size_t()
    _flac_check(lib().d2d_flac_encode_host_effort(channels, bit_depth, effort, buf.ctypes.data, frames, first_block, int(bool(final)),
                                                  out.ctypes.data, cap, C.byref(res), C.byref(used)))
    return out[:res.bytes_out].tobytes(), res, used.value


def flac_encode_device(channels, bit_depth, ios, workspace_ptr, workspace_bytes, stream=None, effort=0):
    """d2d_flac_encode_device_effort: ios is a ctypes array of FlacIO with DEVICE pointers; asynchronous on `stream` (hipStream_t int)."""
    _flac_check(lib().d2d_flac_encode_device_effort(channels, bit_depth, effort, ios, len(ios), C.c_void_p(workspace_ptr), workspace_bytes,
                                                    C.c_void_p(stream or 0)))


def _u8(data):
    import numpy as np
    return np.ascontiguousarray(np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else data.view(np.uint8).reshape(-1))


def flac_decode_host(channels, bit_depth, frames, first_block=0, capacity=None, pcm=None):
    """d2d_flac_decode_host on a bytes-like of whole frames: returns (packed PCM bytes, frames_out, FlacCheck).  `capacity` defaults
    to what 4096 samples per frame byte could never exceed; `pcm` (a uint8 array) is written in place when given."""
    import numpy as np
    buf = _u8(frames)
    fb = channels * (2 if bit_depth == 16 else 3)
    out = pcm if pcm is not None else np.zeros(max((buf.size // 6 + 1) * FLAC_BLOCK * fb if capacity is None else capacity, 1), dtype=np.uint8)
    cap = out.size if capacity is None else capacity
    n, chk = C.c_size_t(), FlacCheck()
    _flac_check(lib().d2d_flac_decode_host(channels, bit_depth, buf.ctypes.data, buf.size, first_block, out.ctypes.data, cap, C.byref(n), C.byref(chk)))
    return out[:n.value * fb].tobytes(), n.value, chk


def flac_verify_host(channels, bit_depth, pcm, out, first_block=0, final=True, sizes=None, method=0, stats=None):
    """d2d_flac_verify_host_method: the frames `out` against the packed PCM they were made from; `sizes` the per-block sizes or None (the
    frames are then walked by decoding); `method` a FLAC_VERIFY_*; `stats` a FlacVerifyStats to fill.  Returns the FlacCheck."""
    import numpy as np
    p, o = _u8(pcm), _u8(out)
    fb = channels * (2 if bit_depth == 16 else 3)
    sz = None if sizes is None else np.ascontiguousarray(np.asarray(sizes, dtype=np.uint32))
    chk = FlacCheck()
    _flac_check(lib().d2d_flac_verify_host_method(channels, bit_depth, p.ctypes.data, p.size // fb if fb else 0, first_block, int(bool(final)),
                                                  o.ctypes.data, o.size, None if sz is None else sz.ctypes.data, C.byref(chk), method,
                                                  None if stats is None else C.byref(stats)))
    return chk


def flac_verify_device(channels, bit_depth, ios, workspace_ptr, workspace_bytes, checks_ptr, stream=None, method=0, stats_ptr=None):
    """d2d_flac_verify_device_method after flac_encode_device on the same ios, workspace and stream; checks_ptr: len(ios) d2d_flac_check
    records (24 bytes each) in memory the GPU can address; stats_ptr: as many d2d_flac_verify_stats (8 bytes each), or None.
    Asynchronous on `stream`."""
    _flac_check(lib().d2d_flac_verify_device_method(channels, bit_depth, method, ios, len(ios), C.c_void_p(workspace_ptr), workspace_bytes,
                                                    C.c_void_p(checks_ptr), C.c_void_p(stats_ptr or 0), C.c_void_p(stream or 0)))


def flac_md5_init_host(n_files=1):
    """d2d_flac_md5_init_host: a ctypes array of n_files fresh FlacMd5State records"""
    states = (FlacMd5State * n_files)()
    lib().d2d_flac_md5_init_host(states, n_files)
    return states


def flac_md5_update_host(channels, bit_depth, pcm, state):
    """d2d_flac_md5_update_host: continues `state` (a FlacMd5State) with a bytes-like of whole interleaved frames; no device"""
    buf = _u8(pcm)
    fb = channels * (2 if bit_depth == 16 else 3)
    _flac_check(lib().d2d_flac_md5_update_host(channels, bit_depth, buf.ctypes.data if buf.size else None, buf.size // fb if fb else 0,
                                               C.byref(state)))


def flac_md5_final_host(state):
    """d2d_flac_md5_final_host: the 16 digest bytes of `state` so far; the state is not modified"""
    digest = (C.c_uint8 * 16)()
    _flac_check(lib().d2d_flac_md5_final_host(C.byref(state), digest))
    return bytes(digest)


def flac_md5_init_device(states_ptr, n_files, stream=None):
    """d2d_flac_md5_init_device: n_files records of 96 bytes at states_ptr (memory the GPU can address); asynchronous on `stream`"""
    _flac_check(lib().d2d_flac_md5_init_device(C.c_void_p(states_ptr), n_files, C.c_void_p(stream or 0)))


def flac_md5_update_device(channels, bit_depth, ios, states_ptr, stream=None):
    """d2d_flac_md5_update_device: ios is a ctypes array of FlacMd5IO with DEVICE pointers; asynchronous on `stream`"""
    _flac_check(lib().d2d_flac_md5_update_device(channels, bit_depth, ios, len(ios), C.c_void_p(states_ptr), C.c_void_p(stream or 0)))


def flac_md5_final_device(states_ptr, n_files, digests_ptr, stream=None):
    """d2d_flac_md5_final_device: 16 digest bytes per file to digests_ptr (memory the GPU can address); asynchronous on `stream`"""
    _flac_check(lib().d2d_flac_md5_final_device(C.c_void_p(states_ptr), n_files, C.c_void_p(digests_ptr), C.c_void_p(stream or 0)))


def loud_coefficients(rate):
    """d2d_loud_coefficients: the ten f64 K-weighting coefficients of `rate` (shelf b0 b1 b2 a1 a2, high-pass b0 b1 b2 a1 a2)"""
    out = (C.c_double * 10)()
    _flac_check(lib().d2d_loud_coefficients(rate, out))
    return list(out)


def loud_measure_host(channels, bit_depth, rate, pcm, first_frame=0, first_subblock=0, final=True, capacity=None):
    """d2d_loud_measure_host on a bytes-like of whole interleaved frames that begin at stream frame `first_frame`: returns (cells, io) --
    cells a float64 array of shape (rows, channels, 2) holding (energy, peak), io the LoudIO with the counts.  No device."""
    import numpy as np
    buf = _u8(pcm)
    fb = channels * (2 if bit_depth == 16 else 4 if bit_depth == 32 else 3)
    frames = buf.size // fb if fb else 0
    if capacity is None:
        capacity = (frames // max(rate // 10, 1) + 2) * max(channels, 1)
    cells = np.zeros((max(capacity, 1), 2), dtype=np.float64)
    io = LoudIO(buf.ctypes.data if buf.size else None, frames, first_frame, first_subblock, int(bool(final)), 0, cells.ctypes.data, capacity, 0, 0, 0)
    _flac_check(lib().d2d_loud_measure_host(channels, bit_depth, rate, C.byref(io)))
    return cells[:io.cells_out].reshape(-1, channels, 2).copy(), io


def loud_measure_device(channels, bit_depth, rate, ios, stream=None):
    """d2d_loud_measure_device: ios is a ctypes array of LoudIO with DEVICE pcm pointers and GPU-addressable cells; asynchronous on
    `stream`; the counts are in ios at return"""
    _flac_check(lib().d2d_loud_measure_device(channels, bit_depth, rate, ios, len(ios), C.c_void_p(stream or 0)))


def true_peak_measure_host(channels, bit_depth, rate, pcm, first_frame=0, first_subblock=0, final=True, capacity=None):
    """d2d_true_peak_measure_host on a bytes-like of whole interleaved frames that begin at stream frame `first_frame`: returns
    (peaks, io) -- peaks a float64 array of shape (rows, channels), io the TruePeakIO with the counts.  No device."""
    import numpy as np
    buf = _u8(pcm)
    fb = channels * (2 if bit_depth == 16 else 4 if bit_depth == 32 else 3)
    frames = buf.size // fb if fb else 0
    if capacity is None:
        capacity = (frames // max(rate // 10, 1) + 2) * max(channels, 1)
    peaks = np.zeros(max(capacity, 1), dtype=np.float64)
    io = TruePeakIO(buf.ctypes.data if buf.size else None, frames, first_frame, first_subblock, int(bool(final)), 0, peaks.ctypes.data, capacity, 0, 0, 0)
    _flac_check(lib().d2d_true_peak_measure_host(channels, bit_depth, rate, C.byref(io)))
    return peaks[:io.peaks_out].reshape(-1, channels).copy(), io


def true_peak_measure_device(channels, bit_depth, rate, ios, stream=None):
    """d2d_true_peak_measure_device: ios is a ctypes array of TruePeakIO with DEVICE pcm pointers and GPU-addressable peaks;
    asynchronous on `stream`; the counts are in ios at return"""
    _flac_check(lib().d2d_true_peak_measure_device(channels, bit_depth, rate, ios, len(ios), C.c_void_p(stream or 0)))


def segments_move_host(segs):
    """d2d_segments_move_host: segs is a ctypes array of Segment with host pointers"""
    _flac_check(lib().d2d_segments_move_host(segs, len(segs)))


def segments_move_device(segs, stream=None):
    """d2d_segments_move_device: segs is a ctypes array of Segment with GPU-addressable pointers; asynchronous on `stream`"""
    _flac_check(lib().d2d_segments_move_device(segs, len(segs), C.c_void_p(stream or 0)))


def segments_pack_host(srcs, dst_ptr, dst_capacity, offsets_ptr):
    """d2d_segments_pack_host: srcs is a ctypes array of PackSrc; offsets_ptr holds len(srcs) + 1 uint64"""
    _flac_check(lib().d2d_segments_pack_host(srcs, len(srcs), C.c_void_p(dst_ptr), dst_capacity, C.c_void_p(offsets_ptr)))


def segments_pack_device(srcs, dst_ptr, dst_capacity, offsets_ptr, stream=None):
    """d2d_segments_pack_device: as the twin, every pointer GPU-addressable, the lengths read on the device; asynchronous on `stream`"""
    _flac_check(lib().d2d_segments_pack_device(srcs, len(srcs), C.c_void_p(dst_ptr), dst_capacity, C.c_void_p(offsets_ptr),
                                               C.c_void_p(stream or 0)))


def _meter_handles(meters):
    return (C.c_void_p * len(meters))(*[m._h.value if m is not None else None for m in meters])


def loud_finish_album(meters):
    """d2d_loud_finish_album: the two gates over the 400 ms blocks of all LoudMeters; returns a LoudResult"""
    r = LoudResult()
    _flac_check(lib().d2d_loud_finish_album(_meter_handles(meters), len(meters), C.byref(r)))
    return r


def loud_true_peak_album(meters):
    """d2d_loud_true_peak_album: the largest d2d_loud_true_peak of the LoudMeters"""
    out = C.c_double()
    _flac_check(lib().d2d_loud_true_peak_album(_meter_handles(meters), len(meters), C.byref(out)))
    return out.value


class LoudMeter:
    """d2d_loud_create / _add / _finish / _destroy: the host integration of one stream's cells (gates, loudness, ReplayGain);
    true_peak=True: d2d_loud_set_true_peak(h, 1) -- add_true_peaks() and true_peak() work, and Engine.convert_stream_flac(loud=)
    measures the true peak too"""

    def __init__(self, channels, rate, weights=None, true_peak=False):
        self._h = C.c_void_p()
        self.channels = channels
        w = (C.c_double * channels)(*weights) if weights is not None else None
        _flac_check(lib().d2d_loud_create(channels, rate, w, C.byref(self._h)))
        if true_peak:
            self.set_true_peak(True)

    def set_true_peak(self, on):
        """d2d_loud_set_true_peak: before the first add"""
        _flac_check(lib().d2d_loud_set_true_peak(self._h, int(bool(on))))

    def add_true_peaks(self, peaks, whole_subblocks=None, has_partial=False):
        """peaks: a float64 array of (rows, channels); every row is a whole sub-block unless has_partial, which makes the last one partial"""
        import numpy as np
        a = np.ascontiguousarray(peaks, dtype=np.float64)
        rows = a.size // self.channels
        if whole_subblocks is None:
            whole_subblocks = rows - (1 if has_partial else 0)
        _flac_check(lib().d2d_loud_add_true_peaks(self._h, a.ctypes.data if a.size else None, whole_subblocks, int(bool(has_partial))))

    def true_peak(self):
        """d2d_loud_true_peak: max(sample peak, largest true-peak value added)"""
        out = C.c_double()
        _flac_check(lib().d2d_loud_true_peak(self._h, C.byref(out)))
        return out.value

    def add(self, cells, whole_subblocks=None, has_partial=False):
        """cells: a float64 array of (rows, channels, 2); every row is a whole sub-block unless has_partial, which makes the last one partial"""
        import numpy as np
        a = np.ascontiguousarray(cells, dtype=np.float64)
        rows = a.size // (2 * self.channels)
        if whole_subblocks is None:
            whole_subblocks = rows - (1 if has_partial else 0)
        _flac_check(lib().d2d_loud_add(self._h, a.ctypes.data if a.size else None, whole_subblocks, int(bool(has_partial))))

    def finish(self):
        r = LoudResult()
        _flac_check(lib().d2d_loud_finish(self._h, C.byref(r)))
        return r

    def close(self):
        if self._h:
            lib().d2d_loud_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class D2DError(Exception):
    def __init__(self, code, message):
        super().__init__(f"[{code}] {message}")
        self.code = code
        self.message = message


def make_params(dsd_rate=1, output_rate=352800, channels=2, fmt="I", endianness="M", block_size=4096,
                filter="E", bit_depth=24, dither="X", level_db=0.0, seed=0, kernel=KERNEL_AUTO, device=0,
                channel_first=0, channel_count=0, tap_bits=0, debug=0):
    """Argument names and defaults follow the reference CLI (src/main.rs:40-110); channel_first/count
    select a channel subset (0 = all), tap_bits the tap grid (0 / 24, or 32), see include/dsd2dxd_amd.h.
    filter: the CLI's letters E, X, D, C, or "S" (FILTER_EQUIRIPPLE_CASCADE): the 48 kHz multiples as stage A
    to 352.8 kHz and a polyphase stage B, where "E" runs the two composed into one pass."""
    return Params(C.sizeof(Params), dsd_rate, output_rate, channels, 1 if fmt.upper() == "P" else 0,
                  1 if endianness.upper() == "M" else 0, block_size, ord(filter.upper()), bit_depth,
                  ord(dither.upper()), kernel, device, level_db, seed, channel_first, channel_count, tap_bits, debug)


class Engine:
    """One conversion context = one Rdsd2Pcm of the reference (src/main.rs:325-342), or a batch of
    `n_files` of them advanced together."""

    def __init__(self, n_files=1, mix=None, half=False, **kw):
        """mix: rows x channels Q15 integers (d2d_create_mix): the engine folds its channels into len(mix) output channels.
        half: d2d_create_half -- output_rate is 44100 or 48000, made by the exact 2:1 decimator behind the FIR of twice that rate"""
        L = lib()
        self.params = make_params(**kw)
        h = C.c_void_p()
        if half:
            if mix is not None:
                raise D2DError(-1, "44100 / 48000 output does not combine with a mix")
            rc = L.d2d_create_half(C.byref(self.params), n_files, C.byref(h))
        elif mix is not None:
            m, keep = _mix_struct(mix, self.params.channels)
            rc = L.d2d_create_mix(C.byref(self.params), C.byref(m), n_files, C.byref(h))
        else:
            rc = L.d2d_create(C.byref(self.params), n_files, C.byref(h))
        if rc:
            raise D2DError(rc, L.d2d_create_error().decode())
        self._h = h
        self.n_files = n_files
        self.channels = self.params.channels                      # width of the INPUT
        self.out_channels = self.params.channel_count or (self.params.channels - self.params.channel_first)
        if mix is not None:
            self.out_channels = m.out_channels
        self.frame_bytes = L.d2d_frame_bytes(h)

    def close(self):
        if getattr(self, "_h", None):
            lib().d2d_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc:
            raise D2DError(rc, lib().d2d_last_error(self._h).decode())

    def info(self):
        i = Info()
        self._check(lib().d2d_get_info(self._h, C.byref(i)))
        return dict(M=i.decimation, ntaps=i.ntaps, S=i.scale_bits, L=i.resamp_L, P=i.resamp_P,
                    kernel=i.kernel, filter=i.filter_name.decode())

    @classmethod
    def create_half(cls, n_files=1, **kw):
        """d2d_create_half: a halved engine (output_rate 44100 or 48000)"""
        return cls(n_files=n_files, half=True, **kw)

    def half_factor(self):
        """2 for an engine of d2d_create_half, else 0"""
        return lib().d2d_half_factor(self._h)

    def get_mix(self):
        """d2d_get_mix: the engine's mix as a list of rows of Q15 integers, or None for an engine that does not mix"""
        rows = C.c_uint32()
        self._check(lib().d2d_get_mix(self._h, C.byref(rows), None, 0))
        if not rows.value:
            return None
        coef = (C.c_int32 * (rows.value * self.channels))()
        self._check(lib().d2d_get_mix(self._h, C.byref(rows), coef, len(coef)))
        return [list(coef[r * self.channels:(r + 1) * self.channels]) for r in range(rows.value)]

    def kernel_name(self):
        return lib().d2d_kernel_name(self._h).decode()

    def dither_table_calls(self):
        """calls so far whose files read their dither words from the per-call table (d2d_dither_table_calls)"""
        return lib().d2d_dither_table_calls(self._h)

    def reset(self):
        self._check(lib().d2d_reset(self._h))

    def next_frames(self, bytes_per_channel, file=0):
        return lib().d2d_next_frames(self._h, file, bytes_per_channel)

    def translate(self, dsd):
        """Host buffers: `dsd` holds channels*bytes_per_channel bytes; returns (uint8 ndarray, frames)."""
        import numpy as np
        buf = np.ascontiguousarray(np.frombuffer(dsd, dtype=np.uint8) if not isinstance(dsd, np.ndarray) else dsd)
        assert buf.size % self.channels == 0
        bpc = buf.size // self.channels
        n = self.next_frames(bpc)
        out = np.zeros(max(n * self.frame_bytes, 1), dtype=np.uint8)
        frames = C.c_size_t()
        self._check(lib().d2d_translate(self._h, buf.ctypes.data, bpc, out.ctypes.data, out.size, C.byref(frames)))
        return out[:frames.value * self.frame_bytes], frames.value

    def translate_into(self, dsd_ptr, bytes_per_channel, pcm_ptr, pcm_capacity_bytes):
        """d2d_translate on raw HOST addresses (e.g. pinned tensors: the kernels then work on them directly); returns frames."""
        frames = C.c_size_t()
        self._check(lib().d2d_translate(self._h, C.c_void_p(dsd_ptr), bytes_per_channel, C.c_void_p(pcm_ptr), pcm_capacity_bytes, C.byref(frames)))
        return frames.value

    def translate_batch_device(self, ios, stream=None):
        """ios: ctypes array of FileIO with DEVICE pointers; asynchronous on `stream` (hipStream_t int)."""
        self._check(lib().d2d_translate_batch_device(self._h, ios, len(ios), C.c_void_p(stream or 0)))

    def translate_batch_host(self, ios, slice_bytes_per_channel=0):
        """ios: ctypes array of FileIO with HOST pointers (pinned for overlap); synchronous."""
        self._check(lib().d2d_translate_batch_host(self._h, ios, len(ios), slice_bytes_per_channel))

    def seek(self, pos, file=0):
        """Put `file` into a fresh engine's state standing at `pos` bytes per channel (d2d_seek); synchronises."""
        self._check(lib().d2d_seek(self._h, file, pos))

    def tell(self, file=0):
        """(bytes per channel consumed, index of the next frame) of `file`"""
        pos, frame = C.c_uint64(), C.c_uint64()
        rc = lib().d2d_tell(self._h, file, C.byref(pos), C.byref(frame))
        if rc:
            raise D2DError(rc, "file out of range")
        return pos.value, frame.value

    def preroll_bytes(self):
        """bytes per channel of halo to prime with before a slice's first byte (d2d_preroll_bytes)"""
        return lib().d2d_preroll_bytes(self._h)

    def slice_align_bytes(self):
        """positions at which a slice may begin are multiples of this (1 unless the dither is noise-shaped)"""
        return lib().d2d_slice_align_bytes(self._h)

    def prime(self, dsd):
        """Host buffer like translate()'s: consumes the bytes, carries the history, produces no frames (d2d_prime)."""
        import numpy as np
        buf = np.ascontiguousarray(np.frombuffer(dsd, dtype=np.uint8) if not isinstance(dsd, np.ndarray) else dsd)
        assert buf.size % self.channels == 0
        self._check(lib().d2d_prime(self._h, buf.ctypes.data, buf.size // self.channels))

    def prime_batch_device(self, ios, stream=None):
        """ios as for translate_batch_device (pcm fields ignored); asynchronous on `stream`."""
        self._check(lib().d2d_prime_batch_device(self._h, ios, len(ios), C.c_void_p(stream or 0)))

    def peak(self, channel, file=0):
        v = C.c_double()
        self._check(lib().d2d_peak(self._h, file, channel, C.byref(v)))
        return v.value

    def peak_dbfs(self, file=0):
        v = C.c_float()
        self._check(lib().d2d_peak_dbfs(self._h, file, C.byref(v)))
        return v.value

    def profile_enable(self, on=True):
        self._check(lib().d2d_profile_enable(self._h, int(on)))

    def profile_read(self):
        ms, n = C.c_double(), C.c_uint64()
        self._check(lib().d2d_profile_read(self._h, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def profile_read_all(self):
        """(FIR kernel ms, whole-call kernels ms, launches) since the last read"""
        fir, step, n = C.c_double(), C.c_double(), C.c_uint64()
        self._check(lib().d2d_profile_read_all(self._h, C.byref(fir), C.byref(step), C.byref(n)))
        return fir.value, step.value, n.value

    def tables_bytes(self):
        return lib().d2d_tables_bytes(self._h)

    def tables_export_device(self, dev_ptr, cap, stream=None):
        self._check(lib().d2d_tables_export_device(self._h, C.c_void_p(dev_ptr), cap, C.c_void_p(stream or 0)))

    def tables_import_device(self, dev_ptr, nbytes, stream=None):
        self._check(lib().d2d_tables_import_device(self._h, C.c_void_p(dev_ptr), nbytes, C.c_void_p(stream or 0)))

    def convert_stream(self, read, write, total_bytes_per_channel=0, chunk_bytes_per_channel=1 << 22,
                       cancel=None, progress=None):
        """do_conversion for callers that own the I/O: read(cap)->bytes (channels*k bytes in layout, k<=cap),
        write(bytes)."""
        keep = {}

        def _read(_u, dst, cap):
            data = read(cap)
            if not data:
                return 0
            n = len(data)
            C.memmove(dst, data, n)
            return n // self.channels

        def _write(_u, p, n):
            write(C.string_at(p, n))
            return 0

        def _prog(_u, pct):
            if progress:
                progress(pct)

        keep["r"], keep["w"], keep["p"] = READ_FN(_read), WRITE_FN(_write), PROGRESS_FN(_prog)
        cflag = cancel if cancel is not None else C.c_int(0)
        self._check(lib().d2d_convert_stream(self._h, keep["r"], None, keep["w"], None, C.byref(cflag),
                                             keep["p"], None, total_bytes_per_channel, chunk_bytes_per_channel))

    def convert_stream_flac(self, read, write, total_bytes_per_channel=0, chunk_bytes_per_channel=1 << 22,
                            cancel=None, progress=None, effort=0, verify=False, md5=False, loud=None):
        """d2d_convert_stream_flac_effort: as convert_stream, but write() receives FLAC frames (whole frames, in order); returns the
        FlacStreamStats STREAMINFO needs.  Errors carry d2d_flac_error()'s message.  verify=True: d2d_convert_stream_flac_verified --
        every chunk's frames are checked against their PCM on the GPU before write() sees them; returns (stats, FlacCheck), and a bad
        block raises D2DError with code ERR_VERIFY (the record so far is the exception's `check`).  md5=True: d2d_convert_stream_flac_md5
        -- the samples are hashed on the GPU as well; the 16 digest bytes for STREAMINFO are returned last: (stats, digest), or with
        verify=True (stats, FlacCheck, digest).  loud=a LoudMeter: d2d_convert_stream_flac_loud -- the samples are also measured on the
        GPU and their cells go into the meter, which the caller finishes; what is returned is what the other switches make it."""
        def _read(_u, dst, cap):
            data = read(cap)
            if not data:
                return 0
            C.memmove(dst, data, len(data))
            return len(data) // self.channels

        def _write(_u, p, n):
            write(C.string_at(p, n))
            return 0

        def _prog(_u, pct):
            if progress:
                progress(pct)

        r, w, p = READ_FN(_read), WRITE_FN(_write), PROGRESS_FN(_prog)
        cflag = cancel if cancel is not None else C.c_int(0)
        stats = FlacStreamStats()
        if loud is not None:
            chk, digest = FlacCheck(), (C.c_uint8 * 16)()
            rc = lib().d2d_convert_stream_flac_loud(self._h, self.params.bit_depth, effort, r, None, w, None, C.byref(cflag), p, None,
                                                    total_bytes_per_channel, chunk_bytes_per_channel, C.byref(stats),
                                                    C.byref(chk) if verify else None, digest if md5 else None, loud._h)
            if rc:
                err = D2DError(rc, lib().d2d_flac_error().decode())
                err.check = chk
                raise err
            out = (stats,) + ((chk,) if verify else ()) + ((bytes(digest),) if md5 else ())
            return out if len(out) > 1 else stats
        if md5:
            chk, digest = FlacCheck(), (C.c_uint8 * 16)()
            rc = lib().d2d_convert_stream_flac_md5(self._h, self.params.bit_depth, effort, r, None, w, None, C.byref(cflag), p, None,
                                                   total_bytes_per_channel, chunk_bytes_per_channel, C.byref(stats),
                                                   C.byref(chk) if verify else None, digest)
            if rc:
                err = D2DError(rc, lib().d2d_flac_error().decode())
                err.check = chk
                raise err
            return (stats, chk, bytes(digest)) if verify else (stats, bytes(digest))
        if verify:
            chk = FlacCheck()
            rc = lib().d2d_convert_stream_flac_verified(self._h, self.params.bit_depth, effort, r, None, w, None, C.byref(cflag), p, None,
                                                        total_bytes_per_channel, chunk_bytes_per_channel, C.byref(stats), C.byref(chk))
            if rc:
                err = D2DError(rc, lib().d2d_flac_error().decode())
                err.check = chk
                raise err
            return stats, chk
        _flac_check(lib().d2d_convert_stream_flac_effort(self._h, self.params.bit_depth, effort, r, None, w, None, C.byref(cflag), p, None,
                                                         total_bytes_per_channel, chunk_bytes_per_channel, C.byref(stats)))
        return stats

    def convert_streams_flac(self, reads, writes, totals=None, chunk_bytes_per_channel=0, cancel=None, progress=None, effort=0,
                             verify=False, md5=False, louds=None):
        """d2d_convert_streams_flac: the engine's n_files streams in lockstep.  reads[f](cap) -> bytes and writes[f](bytes) are file f's
        callbacks (as convert_stream_flac's; a write may be None), louds[f] its LoudMeter or None.  Returns a dict: "stats", "checks"
        (verify) and "md5" (md5) are lists per file, "device_calls" and "chunks" the driver's counts.  A failure raises D2DError with
        d2d_flac_error()'s message; the exception's `ios` are the records so far."""
        n = len(reads)
        ios = (StreamIO * n)()

        def reader(fn):
            def _read(_u, dst, cap):
                data = fn(cap)
                if data is None:
                    return -1
                if not data:
                    return 0
                C.memmove(dst, data, len(data))
                return len(data) // self.channels
            return READ_FN(_read)

        def writer(fn):
            def _write(_u, p, k):
                fn(C.string_at(p, k))
                return 0
            return WRITE_FN(_write)

        for f in range(n):
            ios[f].read = reader(reads[f])
            if writes[f] is not None:
                ios[f].write = writer(writes[f])
            ios[f].total_bytes_per_channel = totals[f] if totals else 0
            ios[f].loud = louds[f]._h if louds and louds[f] is not None else None
        calls, chunks = C.c_uint64(), C.c_uint64()
        cflag = cancel if cancel is not None else C.c_int(0)
        opt = StreamsOptions(C.sizeof(StreamsOptions), self.params.bit_depth, effort, (STREAMS_VERIFY if verify else 0) | (STREAMS_MD5 if md5 else 0),
                             chunk_bytes_per_channel, C.pointer(cflag), PROGRESS_FN(lambda _u, pct: progress(pct) if progress else None),
                             None, C.pointer(calls), C.pointer(chunks))
        rc = lib().d2d_convert_streams_flac(self._h, ios, n, C.byref(opt))
        if rc:
            err = D2DError(rc, lib().d2d_flac_error().decode())
            err.ios = ios
            raise err
        out = {"stats": [ios[f].stats for f in range(n)], "device_calls": calls.value, "chunks": chunks.value}
        if verify:
            out["checks"] = [ios[f].check for f in range(n)]
        if md5:
            out["md5"] = [bytes(ios[f].md5) for f in range(n)]
        out["_keep"] = ios
        return out
