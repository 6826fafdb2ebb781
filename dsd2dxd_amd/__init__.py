"""dsd2dxd_amd -- MI355X-native DSD->PCM decimation engine (drop-in for dsd2dxd's rdsd2pcm path).

The product is the C-ABI shared library `libdsd2dxd_amd.so` (include/dsd2dxd_amd.h), built from
dsd2dxd_amd/csrc for gfx950.  This package is only the thin ctypes binding the tests and bench.py
drive it through; there is no Python or CPU implementation of the conversion behind it.
"""
from ._capi import (D2DError, Engine, FileIO, Info, Params, lib, library_path, build_library,  # noqa: F401
                    KERNEL_AUTO, KERNEL_LUT, KERNEL_MFMA,
                    FILTER_EQUIRIPPLE, FILTER_XLD, FILTER_DSD2PCM, FILTER_CHEBYSHEV, FILTER_EQUIRIPPLE_CASCADE,
                    DBG_NO_MX, DBG_NO_GAINQ, DBG_NO_COOP, DBG_HOST_STAGED, DBG_NO_PIPE, DBG_MFMA_V1, DBG_NO_INTQ, DBG_NS_GENERAL, DBG_TAPS32_2PASS, dbg_waves,
                    DBG_NO_DITHER_TABLE, DITHER_TABLE_MIN_FILES,
                    FLAC_BLOCK, FLAC_EFFORT_FIXED2, FLAC_EFFORT_SEARCH, FLAC_EFFORT_LPC, FlacIO, FlacResult, FlacStreamStats, flac_bound_bytes, flac_workspace_bytes, flac_encode_host, flac_encode_device,
                    FlacCheck, flac_decode_host, flac_verify_host, flac_verify_device, ERR_VERIFY, FLAC_NO_BAD_BLOCK,
                    FlacVerifyStats, FLAC_VERIFY_AUTO, FLAC_VERIFY_SERIAL, FLAC_VERIFY_COOP,
                    FlacMd5State, FlacMd5IO, flac_md5_init_host, flac_md5_update_host, flac_md5_final_host,
                    flac_md5_init_device, flac_md5_update_device, flac_md5_final_device,
                    LoudCell, LoudIO, LoudResult, LoudMeter, loud_coefficients, loud_measure_host, loud_measure_device,
                    TruePeakIO, true_peak_measure_host, true_peak_measure_device,
                    Segment, PackSrc, PACK_GAVE_UP, segments_move_host, segments_move_device, segments_pack_host, segments_pack_device,
                    StreamIO, StreamsOptions, STREAMS_VERIFY, STREAMS_MD5, loud_finish_album, loud_true_peak_album,
                    Mix, MIX_UNITY, mix_preset, mix_frames_host,
                    HalfJob, half_taps, half_frames_host, half_frames_device,
                    MIX_LAYOUT_AUTO, MIX_LAYOUT_STEREO, MIX_LAYOUT_LRC, MIX_LAYOUT_QUAD, MIX_LAYOUT_5_0, MIX_LAYOUT_5_1, MIX_LAYOUT_LRC_LFE,
                    FLAC_BAD_NONE, FLAC_BAD_SIZE, FLAC_BAD_HEADER, FLAC_BAD_CRC8, FLAC_BAD_CRC16, FLAC_BAD_UNSUPPORTED, FLAC_BAD_SYNTAX, FLAC_BAD_LENGTH, FLAC_BAD_SAMPLES)
