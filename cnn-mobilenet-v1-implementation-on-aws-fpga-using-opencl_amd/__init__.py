"""Python mirror of the C-ABI in include/mbn.h (ctypes; no torch types cross the boundary).

The product is the C/HIP library (libmbn.so, built by the Makefile next to this file); this module only
loads it and exposes thin wrappers so tests and bench.py can drive it. There is no CPU fallback:
`load()` raises if the library is missing, and `Context()` raises if there is no HIP device.

The directory name contains '-', so import it with `import_package()` from the repo-root `mbn_amd.py` shim
(or importlib on this file).
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
REPO_ROOT = os.path.dirname(PKG_DIR)
# MBN_LAB=1 in the environment selects the lab build (every A/B variant and mbn_tune_set knob: `make lab`); tools/*.py set it,
# bench.py and the tests run the shipped library unless the caller exports it
# (MBN_LAB=<file name>: another build of the lab library in the package directory — tools' A/B of two source states in one GPU call)
_lab = os.environ.get("MBN_LAB", "")
LIB_PATH = os.path.join(PKG_DIR, "libmbn_lab.so" if _lab == "1" else _lab if (_lab.startswith("libmbn") and _lab.endswith(".so")) else "libmbn.so")
HOST_LIB_PATH = os.path.join(PKG_DIR, "libmbn_host.so")
HEADER = os.path.join(REPO_ROOT, "include", "mbn.h")

RANK_FN = C.CFUNCTYPE(C.c_int, C.c_int, C.c_void_p, C.c_void_p)     # mbn_rank_fn(rank, arg, sync)
OK, EINVAL, ENOMEM, EDEVICE, EIO, EFORMAT, ENOTFOUND, ESHAPE, EUNSUPPORTED, ENODEVICE = 0, -1, -2, -3, -4, -5, -6, -7, -8, -9
DT_U8, DT_F32, DT_BF16, DT_I8 = 0, 1, 2, 3
LAYOUT_NCHW_PLANAR, LAYOUT_NHWC = 0, 1
IO_IN_F32, IO_OUT_F32, IO_IN_U8, IO_FILT_PACKED = 1, 2, 4, 8
ACT_NONE, ACT_RELU, ACT_RELU6 = 0, 1, 2
Q_CARRY_SUM, Q_DW_PLANE0, Q_LITERAL_INDEX, Q_POOL_DIV49 = 1, 2, 4, 8
QUIRKS_NONE, QUIRKS_KERNEL_CL = 0, 0xF
L_CONV, L_DW, L_PW, L_POOL, L_FC = 1, 2, 3, 4, 5
MAX_LAYERS = 32
FIT_STRETCH, FIT_CROP, FIT_PAD = 0, 1, 2
# MBN_FILTER_*: the filter of the resize front-end, PIL.Image.Resampling's own numbers
FILTER_NEAREST, FILTER_LANCZOS, FILTER_BILINEAR, FILTER_BICUBIC, FILTER_BOX, FILTER_HAMMING = 0, 1, 2, 3, 4, 5
FILTER_NAMES = {"nearest": 0, "lanczos": 1, "bilinear": 2, "bicubic": 3, "box": 4, "hamming": 5}


class MbnError(RuntimeError):
    def __init__(self, code, what=""):
        self.code = code
        super().__init__("mbn error %d (%s) %s" % (code, _strerror(code), what))


class BlockParams(C.Structure):
    """mbn_block_params (include/mbn.h): one depthwise + pointwise block of mbn_blocks_resident_bf16"""
    _fields_ = [("wd", C.c_void_p), ("s2", C.c_void_p), ("b2", C.c_void_p), ("wp_bf16", C.c_void_p), ("s3", C.c_void_p), ("b3", C.c_void_p)]


class LayerExt(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("batch", C.c_int32), ("dtype", C.c_int32), ("layout", C.c_int32),
                ("act", C.c_int32), ("pad_top", C.c_int32), ("pad_left", C.c_int32), ("in_rows", C.c_int32),
                ("in_cols", C.c_int32), ("cin", C.c_int32), ("gsize0", C.c_int32), ("gsize1", C.c_int32),
                ("quirks", C.c_uint32), ("quirks_valid", C.c_int32), ("scale", C.c_void_p), ("shift", C.c_void_p),
                ("stream", C.c_void_p), ("io_flags", C.c_int32), ("dilation", C.c_int32)]


class LayerDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("index", "kind", "in_rows", "in_cols", "in_ch", "out_rows", "out_cols",
                                        "out_ch", "stride", "pad_top", "pad_left", "dilation")] + \
               [(n, C.c_int64) for n in ("w_offset", "w_count", "scale_offset", "shift_offset")]


class Plan(C.Structure):
    _fields_ = [("n_layers", C.c_int32), ("res", C.c_int32), ("alpha", C.c_float), ("classes", C.c_int32),
                ("blob_floats", C.c_int64), ("max_act_floats", C.c_int64), ("layer", LayerDesc * MAX_LAYERS)]


class Weights(C.Structure):
    _fields_ = [("plan", Plan), ("blob", C.POINTER(C.c_float))]


class I8Layer(C.Structure):
    """mbn_i8_layer (include/mbn.h): byte offsets of one layer's segments in the i8 blob, and its activation scales"""
    _fields_ = [("w_offset", C.c_int64), ("mult_offset", C.c_int64), ("bias_offset", C.c_int64), ("in_scale", C.c_float),
                ("out_scale", C.c_float)]


class I8Params(C.Structure):
    _fields_ = [("n_layers", C.c_int32), ("blob_bytes", C.c_int64), ("layer", I8Layer * MAX_LAYERS)]


class ResizeItem(C.Structure):
    """mbn_resize_item (include/mbn.h): one image of a ragged resize"""
    _fields_ = [("src_offset", C.c_int64), ("rows", C.c_int32), ("cols", C.c_int32), ("box", C.c_float * 4)]


class LabelItem(C.Structure):
    """mbn_label_item (include/mbn.h): one image of a ragged read-out; dst_offset in elements from labels (and score)"""
    _fields_ = [("dst_offset", C.c_int64), ("rows", C.c_int32), ("cols", C.c_int32)]


class LabelWindowItem(C.Structure):
    """mbn_label_window_item (include/mbn.h): one image of a ragged window read-out: LabelItem and its rectangle (x, y, iw, ih) of the network input"""
    _fields_ = [("dst_offset", C.c_int64)] + [(n, C.c_int32) for n in ("rows", "cols", "x", "y", "iw", "ih")]


ENSEMBLE_MAX_VIEWS = 8


class View(C.Structure):
    """mbn_view (include/mbn.h): one presentation of an image to the network: the rectangle (x, y, iw, ih) of the network input that holds the whole
    image, mirrored left-to-right when mirror = 1; 32 bytes, the reserved words 0"""
    _fields_ = [(n, C.c_int32) for n in ("x", "y", "iw", "ih", "mirror")] + [("reserved", C.c_int32 * 3)]

    @property
    def rect(self):
        return (self.x, self.y, self.iw, self.ih)


SLIDE_MAX_AXIS = 16


class Slide(C.Structure):
    """mbn_slide (include/mbn.h, "segment by sliding window"): a grid of ny x nx tiles of tile_rows x tile_cols at rows y[] and columns x[];
    144 bytes, the unused positions 0"""
    _fields_ = [(n, C.c_int32) for n in ("tile_rows", "tile_cols", "ny", "nx")] + [("y", C.c_int32 * SLIDE_MAX_AXIS), ("x", C.c_int32 * SLIDE_MAX_AXIS)]

    @property
    def ys(self):
        return list(self.y[:self.ny])

    @property
    def xs(self):
        return list(self.x[:self.nx])


class BoundaryMetrics(C.Structure):
    """mbn_boundary_metrics_t (include/mbn.h, "score a segmentation at its boundaries")"""
    _fields_ = [("boundary_miou", C.c_double), ("truth_band_pixels", C.c_double), ("pred_band_pixels", C.c_double),
                ("classes_present", C.c_int32), ("reserved", C.c_int32)]


class SurfaceMetrics(C.Structure):
    """mbn_surface_metrics_t (include/mbn.h, "score a segmentation by surface distance")"""
    _fields_ = [(n, C.c_double) for n in ("hd", "hdp", "assd", "nsd", "n", "unmatched")] + \
               [(n, C.c_int32) for n in ("classes_present", "classes_measurable", "saturated", "reserved")]


class SegMetrics(C.Structure):
    """mbn_seg_metrics (include/mbn.h, "score a segmentation")"""
    _fields_ = [("pixels", C.c_double), ("valid", C.c_double), ("void_pixels", C.c_double), ("abstained", C.c_double),
                ("pixel_accuracy", C.c_double), ("mean_accuracy", C.c_double), ("miou", C.c_double), ("fw_iou", C.c_double),
                ("classes_present", C.c_int32), ("reserved", C.c_int32)]


class Calibration(C.Structure):
    """mbn_calibration (include/mbn.h, "calibration score")"""
    _fields_ = [(n, C.c_double) for n in ("pixels", "answered", "abstained", "void_pixels", "accuracy", "mean_confidence", "ece", "mce", "aurc")]


class Nll(C.Structure):
    """mbn_nll: what mbn_nll_metrics derives from one temperature plane of an NLL table."""
    _fields_ = [(n, C.c_double) for n in ("pixels", "scored", "void_pixels", "nll", "brier", "accuracy", "mean_class_nll", "mean_class_brier")] + \
               [("classes_present", C.c_int)]


class PanopticMetrics(C.Structure):
    """mbn_panoptic_metrics_t (include/mbn.h, "score a segmentation by its regions")"""
    _fields_ = [(n, C.c_double) for n in ("pq", "sq", "rq", "tp", "fp", "fn")] + [("classes_present", C.c_int32), ("reserved", C.c_int32)]


class Region(C.Structure):
    """mbn_region (include/mbn.h, "regions of a label map"): eight int32"""
    _fields_ = [(n, C.c_int32) for n in ("label", "area", "first_row", "first_col", "min_row", "min_col", "max_row", "max_col")]


REGION_DTYPE = np.dtype([(n, np.int32) for n in ("label", "area", "first_row", "first_col", "min_row", "min_col", "max_row", "max_col")])


class ResampleLaunch(C.Structure):
    """mbn_resample_launch_t (host/mbn_envelope.h): LDS footprint, class chunk, dynamic LDS, grid.x and output span of a read-out launch"""
    _fields_ = [(n, C.c_int32) for n in ("fy", "fx", "ch", "lds_bytes", "tiles")] + [("span", C.c_int64)]


class ResizeDesc(C.Structure):
    """mbn_resize_desc (host/mbn_envelope.h): an image's descriptor in device memory, the item and what the host planned for it"""
    _fields_ = [("src_offset", C.c_int64), ("rows", C.c_int32), ("cols", C.c_int32), ("box", C.c_float * 4)] + \
               [(n, C.c_int32) for n in ("kx", "ky", "toh", "tiles_y", "wg0", "seg_stride", "tmp_off", "lds_bytes")]


class ResizePlan(C.Structure):
    """mbn_resize_plan_t (host/mbn_envelope.h): the tile of a resize geometry and its LDS image"""
    _fields_ = [(n, C.c_int32) for n in ("kx", "ky", "tow", "toh", "tiles_x", "tiles_y", "seg_stride", "stage_off", "tmp_off", "lds_bytes")]


class ResizePadPlan(C.Structure):
    """mbn_resize_pad_plan_t (host/mbn_envelope.h): the table plan of a letterbox's inner image, its rectangle and its border workgroups"""
    _fields_ = [("plan", ResizePlan)] + [(n, C.c_int32) for n in ("x", "y", "iw", "ih", "fill_rows", "fill_wgs")]


class ResizePadDesc(C.Structure):
    """mbn_resize_pad_desc (host/mbn_envelope.h): an image's descriptor of a letterbox launch, 96 bytes"""
    _fields_ = [("img", ResizeDesc)] + [(n, C.c_int32) for n in ("x", "y", "iw", "ih", "tow", "tiles_x", "fill_rows", "fill_wgs")]


class I8PwPlan(C.Structure):
    """mbn_i8_pw_plan_t (host/mbn_envelope.h): the launch mbn_launch_i8_pointwise issues for a shape"""
    _fields_ = [(n, C.c_int) for n in ("form", "ks", "g", "out_f32", "pt", "threads", "gy", "lds_bytes")] + \
               [("ntiles", C.c_long), ("gx", C.c_long)] + \
               [(n, C.c_int) for n in ("kp", "cpw", "rep", "resident", "maxg")] + \
               [("per_round", C.c_long), ("rounds", C.c_long)] + \
               [(n, C.c_int) for n in ("nkb", "nchunks", "cpg", "ngroups")]


I8_PW_PERSISTENT, I8_PW_KREG = 1, 2


def build(force: bool = False) -> None:
    """Compile the HIP kernels for gfx950 + the C host (make; hipcc cross-compiles without a GPU): the shipped library and
    the lab build beside it (`all lab`)."""
    args = ["make", "-C", PKG_DIR, "-j8", "all", "lab"]
    if force:
        subprocess.check_call(["make", "-C", PKG_DIR, "clean"], stdout=subprocess.DEVNULL)
    subprocess.check_call(args, stdout=subprocess.DEVNULL)


_lib = None
_host = None


def _declare_host(lib):
    lib.mbn_strerror.restype = C.c_char_p
    lib.mbn_strerror.argtypes = [C.c_int]
    lib.mbn_plan_build.argtypes = [C.c_float, C.c_int, C.c_int, C.POINTER(Plan)]
    lib.mbn_plan_build_hw.argtypes = [C.c_float, C.c_int, C.c_int, C.c_int, C.POINTER(Plan)]
    lib.mbn_plan_build_os.argtypes = [C.c_float, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(Plan)]
    lib.mbn_weights_from_h5.argtypes = [C.c_char_p, C.c_float, C.c_int, C.POINTER(Weights)]
    lib.mbn_weights_from_h5_hw.argtypes = [C.c_char_p, C.c_float, C.c_int, C.c_int, C.POINTER(Weights)]
    lib.mbn_weights_from_h5_os.argtypes = [C.c_char_p, C.c_float, C.c_int, C.c_int, C.c_int, C.POINTER(Weights)]
    lib.mbn_weights_synthetic_h5.argtypes = [C.c_char_p, C.c_float, C.c_int, C.c_uint64]
    lib.mbn_weights_free.argtypes = [C.POINTER(Weights)]
    lib.mbn_h5_open.argtypes = [C.c_char_p, C.POINTER(C.c_void_p)]
    lib.mbn_h5_close.argtypes = [C.c_void_p]
    lib.mbn_h5_get.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_int), C.POINTER(C.c_int64),
                               C.POINTER(C.POINTER(C.c_float))]
    lib.mbn_h5_visit.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.mbn_h5_create.argtypes = [C.c_char_p, C.POINTER(C.c_void_p)]
    lib.mbn_h5_put.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.POINTER(C.c_int64), C.c_void_p]
    lib.mbn_h5_finish.argtypes = [C.c_void_p]
    lib.mbn_read_text_weights.argtypes = [C.c_char_p, C.c_void_p, C.c_int]
    lib.mbn_read_text_weights_f32.argtypes = [C.c_char_p, C.c_void_p, C.c_size_t, C.c_size_t]
    lib.mbn_read_ppm.argtypes = [C.c_char_p, C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int]
    lib.mbn_write_ppm.argtypes = [C.c_char_p, C.c_void_p, C.c_int, C.c_int]
    lib.mbn_split_rgb.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.mbn_softmax_argmax_u8.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_double)]
    lib.readSquezeNetKernel.argtypes = [C.c_void_p, C.c_int]
    lib.readSquezeNetKernel.restype = None
    lib.decode_image.argtypes = [C.c_void_p, C.c_char_p]
    lib.mbn_shard_range.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.mbn_run_ranks.argtypes = [C.c_int, RANK_FN, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
    lib.mbn_rank_barrier.argtypes = [C.c_void_p]
    lib.mbn_rank_fail.argtypes = [C.c_void_p]
    lib.mbn_quantize_i8.argtypes = [C.POINTER(Plan), C.c_void_p, C.c_void_p, C.POINTER(I8Params), C.c_void_p]
    lib.mbn_upsample_argmax_envelope.argtypes = [C.c_int] * 5      # mbn_envelope.h: exported, not in mbn.h
    lib.mbn_resample_argmax_envelope.argtypes = [C.c_int] * 6      # mbn_envelope.h, like the two below
    lib.mbn_softmax_readout_check.argtypes = [C.c_int, C.c_float]
    lib.mbn_resample_plan.argtypes = [C.c_int] * 4 + [C.POINTER(ResampleLaunch)]
    lib.mbn_resample_plan.restype = None
    lib.mbn_resample_ragged_check.argtypes = [C.c_int] * 3 + [C.POINTER(LabelItem), C.c_int, C.POINTER(C.c_int64), C.POINTER(ResampleLaunch)]
    lib.mbn_resample_window_envelope.argtypes = [C.c_int] * 6 + [C.POINTER(C.c_int32), C.c_int, C.c_int]
    lib.mbn_resample_window_plan.argtypes = [C.c_int] * 4 + [C.POINTER(C.c_int32), C.c_int, C.c_int, C.POINTER(ResampleLaunch)]
    lib.mbn_resample_window_plan.restype = None
    lib.mbn_fit_view.argtypes = [C.c_int] * 4 + [C.c_float, C.c_int, C.POINTER(View)]
    lib.mbn_resample_ensemble_envelope.argtypes = [C.c_int] * 6 + [C.POINTER(View), C.c_int, C.c_int, C.c_int]      # mbn_envelope.h, like the next two
    lib.mbn_resample_ensemble_plan.argtypes = [C.c_int] * 4 + [C.POINTER(View), C.c_int, C.c_int, C.c_int, C.POINTER(ResampleLaunch)]
    lib.mbn_slide_axis.argtypes = [C.c_int] * 3 + [C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    lib.mbn_slide_plan.argtypes = [C.c_int] * 6 + [C.POINTER(Slide)]
    lib.mbn_slide_check.argtypes = [C.POINTER(Slide), C.c_int, C.c_int]                                            # mbn_envelope.h, like the next two
    lib.mbn_resample_slide_envelope.argtypes = [C.c_int] * 4 + [C.POINTER(Slide), C.c_int, C.c_int]
    lib.mbn_resample_slide_plan.argtypes = [C.c_int, C.c_int, C.POINTER(Slide), C.c_int, C.c_int, C.POINTER(ResampleLaunch)]
    lib.mbn_resize_view_table_plan_filter.argtypes = [C.c_int] * 5 + [C.POINTER(View), C.POINTER(ResizePadPlan)]
    lib.mbn_resample_ragged_window_check.argtypes = [C.c_int] * 5 + [C.POINTER(LabelWindowItem), C.c_int, C.POINTER(C.c_int64),
                                                                     C.POINTER(ResampleLaunch)]
    lib.mbn_confusion_envelope.argtypes = [C.c_int, C.c_int, C.c_int64]
    lib.mbn_confusion_form.argtypes = [C.c_int]
    lib.mbn_confusion_metrics.argtypes = [C.POINTER(C.c_uint64), C.c_int, C.POINTER(SegMetrics), C.POINTER(C.c_double)]
    lib.mbn_resample_topk_envelope.argtypes = [C.c_int] * 6 + [C.POINTER(C.c_int32)] + [C.c_int] * 3
    lib.mbn_resample_topk_ragged_check.argtypes = [C.c_int, C.c_int64, C.c_int, C.c_int64]                        # mbn_envelope.h, like the next two
    lib.mbn_topk_rank_envelope.argtypes = [C.c_int, C.c_int, C.c_int64, C.c_int, C.c_int64]
    lib.mbn_topk_rank_form.argtypes = [C.c_int, C.c_int]
    lib.mbn_topk_metrics.argtypes = [C.POINTER(C.c_uint64), C.c_int, C.c_int] + [C.POINTER(C.c_double)] * 3
    lib.mbn_calibration_envelope.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int64]
    lib.mbn_calibration_metrics.argtypes = [C.POINTER(C.c_uint64), C.c_int, C.POINTER(Calibration)] + [C.POINTER(C.c_double)] * 4
    lib.mbn_calibration_threshold.argtypes = [C.POINTER(C.c_uint64), C.c_int, C.c_double, C.POINTER(C.c_float)] + [C.POINTER(C.c_double)] * 2
    lib.mbn_resample_nll_envelope.argtypes = [C.c_int] * 6 + [C.POINTER(C.c_int32)] + [C.c_int] * 4
    lib.mbn_resample_nll_ragged_check.argtypes = [C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int64]              # mbn_envelope.h, like the next
    lib.mbn_nll_temps_check.argtypes = [C.POINTER(C.c_float), C.c_int]
    lib.mbn_nll_metrics.argtypes = [C.POINTER(C.c_uint64), C.c_int, C.c_int, C.c_int, C.POINTER(Nll)] + [C.POINTER(C.c_double)] * 2
    lib.mbn_nll_best.argtypes = [C.POINTER(C.c_uint64), C.c_int, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_int), C.POINTER(C.c_double),
                                 C.POINTER(C.c_int)]
    lib.mbn_components_envelope.argtypes = [C.c_int] * 7
    lib.mbn_components_tile.argtypes = [C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.mbn_components_scratch_bytes.argtypes = [C.c_int, C.c_int64]
    lib.mbn_components_scratch_bytes.restype = C.c_int64
    lib.mbn_panoptic_envelope.argtypes = [C.c_int] * 6
    lib.mbn_panoptic_scratch_bytes.argtypes = [C.c_int, C.c_int64]
    lib.mbn_panoptic_scratch_bytes.restype = C.c_int64
    lib.mbn_panoptic_metrics.argtypes = [C.POINTER(C.c_uint64), C.c_int, C.POINTER(PanopticMetrics)] + [C.POINTER(C.c_double)] * 3
    lib.mbn_boundary_d.argtypes = [C.c_int, C.c_int, C.c_double]
    lib.mbn_boundary_envelope.argtypes = [C.c_int] * 7
    lib.mbn_boundary_tile.argtypes = [C.c_int] + [C.POINTER(C.c_int)] * 3
    lib.mbn_boundary_metrics.argtypes = [C.POINTER(C.c_uint64), C.c_int, C.POINTER(BoundaryMetrics), C.POINTER(C.c_double)]
    lib.mbn_surface_envelope.argtypes = [C.c_int] * 7
    lib.mbn_surface_tile.argtypes = [C.POINTER(C.c_int)] * 2
    lib.mbn_surface_scratch_bytes.argtypes = [C.c_int, C.c_int64, C.c_int]
    lib.mbn_surface_scratch_bytes.restype = C.c_int64
    lib.mbn_surface_metrics.argtypes = [C.POINTER(C.c_uint64), C.c_int, C.c_int, C.c_int, C.c_double, C.POINTER(SurfaceMetrics)] + \
                                       [C.POINTER(C.c_double)] * 4
    i32p = C.POINTER(C.c_int32)
    lib.mbn_resize_ksize.argtypes = [C.c_int, C.c_float, C.c_float, C.c_int]
    lib.mbn_resize_taps.argtypes = [C.c_int, C.c_float, C.c_float, C.c_int, i32p, i32p, i32p]
    lib.mbn_fit_box.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.POINTER(C.c_float)]
    lib.mbn_resize_envelope.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_float), C.c_int, C.c_int]      # mbn_envelope.h: exported, not in mbn.h
    lib.mbn_i8_pw_plan.argtypes = [C.c_long, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(I8PwPlan)]
    lib.mbn_resize_window.argtypes = [C.c_int, C.c_float, C.c_float, C.c_int, C.c_int, C.c_int, i32p, i32p]      # mbn_envelope.h, like the three below
    lib.mbn_resize_table_plan.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_float), C.c_int, C.c_int, C.POINTER(ResizePlan)]
    lib.mbn_resize_ragged_plan.argtypes = [C.POINTER(ResizeItem), C.c_int, C.c_int, C.POINTER(ResizeDesc)]
    lib.mbn_resize_ragged_plan_batch.argtypes = [C.POINTER(ResizeItem), C.c_int, C.c_int, C.c_int, C.POINTER(ResizeDesc), i32p, i32p, C.POINTER(C.c_int64)]
    # the same under a filter (MBN_FILTER_*): the filter is the first argument
    lib.mbn_resize_ksize_filter.argtypes = [C.c_int] + lib.mbn_resize_ksize.argtypes
    lib.mbn_resize_taps_filter.argtypes = [C.c_int] + lib.mbn_resize_taps.argtypes
    lib.mbn_resize_nearest_index.argtypes = [C.c_int, C.c_float, C.c_float, C.c_int, i32p]
    lib.mbn_resize_envelope_filter.argtypes = [C.c_int] + lib.mbn_resize_envelope.argtypes
    lib.mbn_resize_window_filter.argtypes = [C.c_int] + lib.mbn_resize_window.argtypes
    lib.mbn_resize_table_plan_filter.argtypes = [C.c_int] + lib.mbn_resize_table_plan.argtypes
    lib.mbn_resize_ragged_plan_filter.argtypes = [C.c_int] + lib.mbn_resize_ragged_plan.argtypes
    lib.mbn_resize_ragged_plan_batch_filter.argtypes = [C.c_int] + lib.mbn_resize_ragged_plan_batch.argtypes
    # the letterbox (MBN_FIT_PAD): the rectangle, and the plans of its two launches
    lib.mbn_fit_pad.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, i32p]
    lib.mbn_resize_pad_table_plan_filter.argtypes = [C.c_int] * 5 + [C.POINTER(ResizePadPlan)]
    lib.mbn_resize_pad_ragged_plan_filter.argtypes = [C.c_int, C.POINTER(ResizeItem), C.c_int, C.c_int, C.POINTER(ResizePadDesc)]
    lib.mbn_resize_pad_ragged_plan_batch_filter.argtypes = [C.c_int, C.POINTER(ResizeItem), C.c_int, C.c_int, C.c_int, C.POINTER(ResizePadDesc), i32p, i32p,
                                                            C.POINTER(C.c_int64)]
    return lib


def host_lib():
    """The C host alone (no HIP): plan, loaders, .h5 reader/writer. Usable on a CPU-only box."""
    global _host
    if _host is None:
        if not os.path.exists(HOST_LIB_PATH):
            raise FileNotFoundError("%s missing: run __graft_entry__.build() / make" % HOST_LIB_PATH)
        _host = _declare_host(C.CDLL(HOST_LIB_PATH))
    return _host


def load():
    """Load libmbn.so (HIP kernels + C-ABI + C host). Raises if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise FileNotFoundError("%s missing: the HIP extension is not built (no fallback exists)" % LIB_PATH)
        lib = _declare_host(C.CDLL(LIB_PATH))
        vp, ci = C.c_void_p, C.c_int
        lib.mbn_version.restype = C.c_char_p
        lib.mbn_last_device_error.restype = C.c_char_p
        lib.mbn_last_device_error.argtypes = [vp]
        lib.mbn_init.argtypes = [ci, C.POINTER(vp)]
        lib.mbn_shutdown.argtypes = [vp]
        lib.mbn_device_count.argtypes = [C.POINTER(ci)]
        lib.mbn_device_name.argtypes = [vp, C.c_char_p, C.c_size_t]
        lib.mbn_device_cus.argtypes = [vp, C.POINTER(C.c_int)]
        lib.mbn_set_planning_cus.argtypes = [vp, ci]
        lib.mbn_device_pci_bus_id.argtypes = [vp, C.c_char_p, C.c_size_t]
        lib.mbn_pw_clock_read.argtypes = [vp, ci, C.POINTER(C.c_double), C.POINTER(C.c_longlong)]
        lib.mbn_set_literal_quirks.argtypes = [vp, C.c_uint32]
        lib.mbn_get_stream.argtypes = [vp, C.POINTER(vp)]
        lib.mbn_alloc.argtypes = [vp, C.c_size_t, C.POINTER(vp)]
        lib.mbn_free.argtypes = [vp, vp]
        lib.mbn_upload.argtypes = [vp, vp, vp, C.c_size_t]
        lib.mbn_download.argtypes = [vp, vp, vp, C.c_size_t]
        lib.mbn_memset.argtypes = [vp, vp, ci, C.c_size_t]
        lib.mbn_sync.argtypes = [vp]
        lib.mbn_last_kernel_ms.argtypes = [vp, C.POINTER(C.c_float)]
        lib.mbn_set_profiling.argtypes = [vp, ci]
        lib.mbn_profile_begin.argtypes = [vp, ci]
        lib.mbn_profile_end.argtypes = [vp, C.POINTER(C.c_float), ci, C.POINTER(ci)]
        lib.mbn_profile_pause.argtypes = [vp, ci]
        lib.mbn_profile_null.argtypes = [vp, ci, vp]
        lib.mbn_mark.argtypes = [vp, vp]
        lib.mbn_dist_init.argtypes = [ci, C.POINTER(ci), C.POINTER(vp)]
        lib.mbn_dist_size.argtypes = [vp, C.POINTER(ci)]
        lib.mbn_dist_context.argtypes = [vp, ci, C.POINTER(vp)]
        lib.mbn_dist_broadcast.argtypes = [vp, C.POINTER(vp), C.c_size_t, ci]
        lib.mbn_dist_sync.argtypes = [vp]
        lib.mbn_dist_shutdown.argtypes = [vp]
        lib.mbn_dist_last_error.restype = C.c_char_p
        lib.mbn_dist_last_error.argtypes = [vp]
        lib.mbn_marks_read.argtypes = [vp, C.POINTER(C.c_float), ci, C.POINTER(ci)]
        ext = C.POINTER(LayerExt)
        lib.mbn_convolute.argtypes = [vp, vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, ext]
        lib.mbn_depthwise.argtypes = [vp, vp, vp, vp, ci, ci, ci, ci, ci, ext]
        lib.mbn_pointwise.argtypes = [vp, vp, vp, vp, ci, ci, ci, ci, ext]
        lib.mbn_pool.argtypes = [vp, vp, vp, ci, ci, ci, ci, ext]
        lib.mbn_softmax_f32.argtypes = [vp, vp, vp, vp, ci, ci, vp]
        lib.mbn_normalize_u8_to_f32.argtypes = [vp, vp, vp, C.c_size_t, C.c_float, C.c_float, vp]
        lib.mbn_convert_f32_to_bf16.argtypes = [vp, vp, vp, C.c_size_t, vp]
        lib.mbn_packed_filter_offset.restype = C.c_size_t
        lib.mbn_packed_filter_offset.argtypes = [ci, ci]
        lib.mbn_pack_filter_bf16.argtypes = [vp, vp, ci, ci, vp]
        lib.mbn_convert_bf16_to_f32.argtypes = [vp, vp, vp, C.c_size_t, vp]
        lib.mbn_net_set_dtype.argtypes = [vp, ci]
        lib.mbn_net_set_act_scales_i8.argtypes = [vp, C.POINTER(C.c_float), ci]
        lib.mbn_net_get_act_scales_i8.argtypes = [vp, C.POINTER(C.c_float), ci]
        lib.mbn_net_calibrate_i8.argtypes = [vp, vp, ci]
        lib.mbn_tune_set.argtypes = [C.c_char_p, ci]
        lib.mbn_tune_get.argtypes = [C.c_char_p, C.POINTER(ci)]
        lib.mbn_net_set_streams.argtypes = [vp, ci]
        lib.mbn_net_set_free_running.argtypes = [vp, ci]
        lib.mbn_net_set_graph.argtypes = [vp, ci]
        lib.mbn_net_set_fuse_stem.argtypes = [vp, ci]
        lib.mbn_net_fused_layers.argtypes = [vp, ci, C.POINTER(ci)]
        lib.mbn_net_set_fuse_blocks.argtypes = [vp, C.c_uint]
        lib.mbn_net_get_fuse_blocks.argtypes = [vp, C.POINTER(C.c_uint)]
        lib.mbn_net_reset_fuse_blocks.argtypes = [vp]
        lib.mbn_net_set_fuse_tail.argtypes = [vp, ci]
        lib.mbn_pool_fc_workspace_bytes.argtypes = [ci, ci]
        lib.mbn_pool_fc_workspace_bytes.restype = C.c_size_t
        lib.mbn_pool_fc.argtypes = [vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, vp, C.c_size_t, vp]
        lib.mbn_classifier_tail_fused.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, vp, C.c_size_t, vp]
        lib.mbn_forget.argtypes = [vp, vp, C.c_size_t]
        lib.mbn_net_classify.argtypes = [vp, vp, ci, ci, vp, vp]
        lib.mbn_net_launches.argtypes = [vp, ci, ci, C.POINTER(ci), C.POINTER(ci), ci, C.POINTER(ci)]
        lib.mbn_stem_fused.argtypes = [vp] + [vp] * 11 + [ci, ci, ci, ci, vp]
        lib.mbn_stem_fused_u8.argtypes = [vp] + [vp] * 11 + [ci, ci, ci, ci, vp]
        lib.mbn_stem_fused_ex.argtypes = [vp] + [vp] * 11 + [ci, ci, ci, ci, ci, vp]
        lib.mbn_stem_fused_hw.argtypes = [vp] + [vp] * 11 + [ci, ci, ci, ci, ci, ci, vp]
        lib.mbn_net_set_input_u8.argtypes = [vp, ci]
        lib.mbn_net_set_fuse_resident.argtypes = [vp, ci]
        lib.mbn_dwpw_fused.argtypes = [vp] + [vp] * 8 + [ci] * 10 + [vp]
        lib.mbn_dwpw_fused_bf16.argtypes = [vp] + [vp] * 8 + [ci] * 10 + [vp]
        lib.mbn_blocks_resident_bf16.argtypes = [vp, vp, vp, C.POINTER(BlockParams), ci, ci, ci, ci, ci, vp]
        lib.mbn_tail_resident_bf16.argtypes = [vp, vp, vp, C.POINTER(BlockParams), ci, ci, ci, ci, ci, vp]
        lib.mbn_softmax_topk_f32.argtypes = [vp, vp, vp, vp, vp, ci, ci, ci, vp]
        lib.mbn_classifier_tail.argtypes = [vp] * 9 + [ci] * 6 + [vp]
        lib.mbn_upsample_argmax_f32.argtypes = [vp, vp, vp, vp, ci, ci, ci, ci, ci, vp]
        lib.mbn_net_forward_dense.argtypes = [vp, vp, vp, ci]
        lib.mbn_net_segment.argtypes = [vp, vp, ci, vp, vp]
        lib.mbn_resample_argmax_f32.argtypes = [vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, vp]
        lib.mbn_ragged_readout_create.argtypes = [vp, ci, C.POINTER(vp)]
        lib.mbn_ragged_readout_set.argtypes = [vp, ci, ci, ci, C.POINTER(LabelItem), ci, vp]
        lib.mbn_resample_argmax_ragged_f32.argtypes = [vp, vp, vp, vp, vp]
        lib.mbn_ragged_readout_destroy.argtypes = [vp]
        lib.mbn_resample_argmax_window_f32.argtypes = [vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, C.POINTER(C.c_int32), ci, ci, vp]
        lib.mbn_ragged_readout_set_window.argtypes = [vp, ci, ci, ci, ci, ci, C.POINTER(LabelWindowItem), ci, vp]
        lib.mbn_net_segment_fit.argtypes = [vp, vp, ci, ci, ci, ci, vp, vp]
        lib.mbn_net_segment_images_fit.argtypes = [vp, vp, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_int32), ci, ci, vp,
                                                   C.POINTER(C.c_int64), vp]
        lib.mbn_net_segment_to.argtypes = [vp, vp, ci, ci, ci, vp, vp]
        lib.mbn_resample_softmax_f32.argtypes = [vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, C.c_float, ci, vp]
        lib.mbn_resample_softmax_window_f32.argtypes = [vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, C.POINTER(C.c_int32), ci, ci, C.c_float, ci, vp]
        lib.mbn_resample_softmax_ragged_f32.argtypes = [vp, vp, vp, vp, vp, C.c_float, ci, vp]
        lib.mbn_net_segment_prob_to.argtypes = [vp, vp, ci, ci, ci, vp, vp, C.c_float, ci]
        lib.mbn_net_segment_prob_fit.argtypes = [vp, vp, ci, ci, ci, ci, vp, vp, C.c_float, ci]
        lib.mbn_net_segment_prob_images_fit.argtypes = [vp, vp, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_int32), ci, ci, vp,
                                                        C.POINTER(C.c_int64), vp, C.c_float, ci]
        lib.mbn_net_segment_images.argtypes = [vp, vp, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_int32), ci, vp, C.POINTER(C.c_int64), vp]
        lib.mbn_resample_ensemble_f32.argtypes = [vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, C.POINTER(View), ci, ci, ci, C.c_float, ci, vp]
        lib.mbn_resample_slide_f32.argtypes = [vp, vp, vp, vp, vp, ci, ci, ci, ci, C.POINTER(Slide), ci, ci, C.c_float, ci, vp]
        lib.mbn_net_resize_tiles.argtypes = [vp, vp, ci, ci, ci, C.POINTER(Slide), C.POINTER(vp)]
        lib.mbn_net_segment_slide.argtypes = [vp, vp, ci, ci, ci, ci, ci, ci, ci, vp, vp, vp, C.c_float, ci]
        lib.mbn_resizer_create_view.argtypes = [vp, ci, ci, ci, ci, ci, C.POINTER(View), C.POINTER(C.c_uint8), C.POINTER(vp)]
        lib.mbn_net_resize_views.argtypes = [vp, vp, ci, ci, ci, C.POINTER(C.c_float), C.POINTER(C.c_int32), ci, C.POINTER(vp)]
        lib.mbn_net_segment_views_fit.argtypes = [vp, vp, ci, ci, ci, C.POINTER(C.c_float), C.POINTER(C.c_int32), ci, vp, vp, vp, C.c_float, ci]
        lib.mbn_confusion_i32.argtypes = [vp, vp, vp, vp, ci, ci, C.c_int64, vp]
        lib.mbn_confusion_ragged_i32.argtypes = [vp, vp, vp, vp, ci, ci, vp]
        lib.mbn_net_segment_score.argtypes = [vp, vp, vp, ci, vp]
        lib.mbn_resample_topk_f32.argtypes = [vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, C.POINTER(C.c_int32), ci, ci, ci, C.c_float, ci, vp]
        lib.mbn_resample_topk_ragged_f32.argtypes = [vp, vp, vp, vp, vp, ci, C.c_int64, C.c_float, ci, vp]
        lib.mbn_topk_rank_i32.argtypes = [vp, vp, vp, ci, C.c_int64, vp, ci, ci, C.c_int64, vp]
        lib.mbn_topk_rank_ragged_i32.argtypes = [vp, vp, vp, ci, C.c_int64, vp, ci, ci, vp]
        lib.mbn_calibration_f32.argtypes = [vp, vp, vp, vp, vp, ci, ci, ci, C.c_int64, vp]
        lib.mbn_calibration_ragged_f32.argtypes = [vp, vp, vp, vp, vp, ci, ci, ci, vp]
        lib.mbn_net_segment_calibration.argtypes = [vp, vp, vp, vp, ci, ci, vp]
        lib.mbn_resample_nll_f32.argtypes = [vp, vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, ci, C.POINTER(C.c_int32), ci, ci, C.POINTER(C.c_float), ci, vp]
        lib.mbn_resample_nll_ragged_f32.argtypes = [vp, vp, vp, vp, C.c_int64, vp, vp, ci, C.POINTER(C.c_float), ci, vp]
        lib.mbn_net_segment_nll.argtypes = [vp, vp, ci, C.POINTER(C.c_float), ci, vp, vp, vp, C.c_int64]
        lib.mbn_net_segment_topk_fit.argtypes = [vp, vp, ci, ci, ci, ci, ci, vp, vp, vp, C.c_float, ci]
        lib.mbn_net_segment_topk_images_fit.argtypes = [vp, vp, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_int32), ci, ci, ci, C.c_int64,
                                                        vp, C.POINTER(C.c_int64), vp, vp, C.c_float, ci]
        lib.mbn_net_segment_topk_score.argtypes = [vp, vp, vp, ci, vp]
        lib.mbn_components_create.argtypes = [vp, ci, C.c_int64, C.POINTER(vp)]
        lib.mbn_components_destroy.argtypes = [vp]
        lib.mbn_components_i32.argtypes = [vp, vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, ci, ci, vp]
        lib.mbn_components_ragged_i32.argtypes = [vp, vp, vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, vp]
        lib.mbn_net_segment_regions.argtypes = [vp, vp, vp, vp, vp, vp, ci, ci, ci, ci]
        lib.mbn_panoptic_create.argtypes = [vp, ci, C.c_int64, C.POINTER(vp)]
        lib.mbn_panoptic_destroy.argtypes = [vp]
        lib.mbn_panoptic_i32.argtypes = [vp] * 10 + [ci] + [vp] * 3 + [ci] * 5 + [vp]
        lib.mbn_panoptic_ragged_i32.argtypes = [vp] * 11 + [ci] + [vp] * 3 + [ci] * 2 + [vp]
        lib.mbn_widen_u8_i32.argtypes = [vp, vp, vp, C.c_int64, vp]
        lib.mbn_ragged_readout_span.argtypes = [vp]
        lib.mbn_ragged_readout_span.restype = C.c_int64
        lib.mbn_net_set_panoptic_regions.argtypes = [vp, ci]
        lib.mbn_net_segment_panoptic.argtypes = [vp, vp, vp, ci, ci, ci, vp, vp]
        lib.mbn_boundary_d_items.argtypes = [vp, C.c_double, C.POINTER(C.c_int32)]
        lib.mbn_boundary_depth.argtypes = [vp, vp, vp, ci, ci, ci, ci, ci, ci, vp]
        lib.mbn_boundary_depth_ragged.argtypes = [vp, vp, vp, ci, ci, vp, ci, vp]
        lib.mbn_boundary_score_i32.argtypes = [vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, ci, vp]
        lib.mbn_boundary_score_ragged_i32.argtypes = [vp, vp, vp, vp, vp, ci, ci, ci, vp, ci, vp]
        lib.mbn_net_segment_boundary_score.argtypes = [vp, vp, vp, ci, vp, vp, C.c_double, ci, ci]
        lib.mbn_net_segment_boundary_depth.argtypes = [vp, vp, vp, C.c_double, ci, ci]
        lib.mbn_surface_create.argtypes = [vp, ci, C.c_int64, ci, C.POINTER(vp)]
        lib.mbn_surface_destroy.argtypes = [vp]
        lib.mbn_surface_score_i32.argtypes = [vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, ci, vp]
        lib.mbn_surface_score_ragged_i32.argtypes = [vp, vp, vp, vp, vp, vp, ci, ci, ci, ci, vp]
        lib.mbn_net_segment_surface.argtypes = [vp, vp, vp, ci, ci, ci, vp, vp]
        lib.mbn_resizer_create.argtypes = [vp, ci, ci, C.POINTER(C.c_float), ci, ci, C.POINTER(vp)]
        lib.mbn_resize_u8.argtypes = [vp, vp, vp, ci, vp]
        lib.mbn_resizer_destroy.argtypes = [vp]
        lib.mbn_net_resize_input.argtypes = [vp, vp, ci, ci, ci, ci, C.c_float, C.POINTER(vp)]
        lib.mbn_ragged_resizer_create.argtypes = [vp, ci, ci, ci, C.POINTER(vp)]
        lib.mbn_ragged_resizer_set.argtypes = [vp, C.POINTER(ResizeItem), ci, vp]
        lib.mbn_resize_ragged_u8.argtypes = [vp, vp, vp, vp]
        lib.mbn_ragged_resizer_destroy.argtypes = [vp]
        lib.mbn_resize_taps_device.argtypes = [vp, ci, C.c_float, C.c_float, ci, vp, vp, vp]
        lib.mbn_net_resize_inputs.argtypes = [vp, vp, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_int32), ci, ci, C.c_float, C.POINTER(vp)]
        lib.mbn_resizer_create_filter.argtypes = [vp, ci, ci, ci, C.POINTER(C.c_float), ci, ci, C.POINTER(vp)]
        lib.mbn_ragged_resizer_create_filter.argtypes = [vp, ci, ci, ci, ci, C.POINTER(vp)]
        lib.mbn_resize_taps_device_filter.argtypes = [vp, ci, ci, C.c_float, C.c_float, ci, vp, vp, vp]
        lib.mbn_net_set_resize_filter.argtypes = [vp, ci]
        lib.mbn_net_get_resize_filter.argtypes = [vp, C.POINTER(ci)]
        u8p = C.POINTER(C.c_uint8)
        lib.mbn_resizer_create_pad.argtypes = [vp, ci, ci, ci, ci, ci, u8p, C.POINTER(vp)]
        lib.mbn_ragged_resizer_create_pad.argtypes = [vp, ci, ci, ci, ci, u8p, C.POINTER(vp)]
        lib.mbn_net_set_pad_color.argtypes = [vp, ci, ci, ci]
        lib.mbn_net_get_pad_color.argtypes = [vp, C.POINTER(ci), C.POINTER(ci), C.POINTER(ci)]
        lib.mbn_graph_begin.argtypes = [vp, vp]
        lib.mbn_graph_end.argtypes = [vp, vp, C.POINTER(vp)]
        lib.mbn_graph_launch.argtypes = [vp, vp, vp]
        lib.mbn_graph_destroy.argtypes = [vp, vp]
        lib.mbn_stream_create.argtypes = [vp, C.POINTER(vp)]
        lib.mbn_stream_destroy.argtypes = [vp, vp]
        lib.mbn_stream_wait.argtypes = [vp, vp, vp]
        lib.mbn_net_create.argtypes = [vp, C.POINTER(Weights), ci, C.POINTER(vp)]
        lib.mbn_net_create_from_device_blob.argtypes = [vp, C.POINTER(Plan), vp, ci, C.POINTER(vp)]
        lib.mbn_net_destroy.argtypes = [vp]
        lib.mbn_net_forward.argtypes = [vp, vp, vp, ci, ci]
        lib.mbn_net_forward_timed.argtypes = [vp, vp, vp, ci, C.POINTER(C.c_float), ci]
        lib.mbn_net_plan.argtypes = [vp, C.POINTER(Plan)]
        lib.mbn_net_set_keep_activations.argtypes = [vp, ci]
        lib.mbn_net_layer_output.argtypes = [vp, ci, C.POINTER(vp), C.POINTER(C.c_size_t)]
        _lib = lib
    return _lib


def _strerror(code):
    for l in (_lib, _host):
        if l is not None:
            return l.mbn_strerror(code).decode()
    return "?"


def _chk(rc, what=""):
    if rc != OK:
        raise MbnError(rc, what)


def i8_pw_plan(m, cin, op_size, num_cus, operands_on_16=True, out_f32=False, lib=None) -> I8PwPlan:
    """mbn_i8_pw_plan: the launch of an int8 pointwise call of m pixels, K = cin, N = op_size on a device of num_cus CUs."""
    p = I8PwPlan()
    _chk((lib or host_lib()).mbn_i8_pw_plan(m, cin, op_size, num_cus, int(operands_on_16), int(out_f32), C.byref(p)),
         "i8_pw_plan(%d, %d, %d)" % (m, cin, op_size))
    return p


def _box4(box):
    """A box (left, upper, right, lower) as a C float[4], or None for the whole image."""
    if box is None:
        return None
    return (C.c_float * 4)(*[float(np.float32(v)) for v in box])


def resize_ksize(in_size, b0, b1, out_size, lib=None, filter=FILTER_BILINEAR) -> int:
    """mbn_resize_ksize_filter: taps per output of one axis of the resize front-end (raises MbnError on a refused box or filter)."""
    k = (lib or host_lib()).mbn_resize_ksize_filter(filter, in_size, b0, b1, out_size)
    if k < 0:
        raise MbnError(k, "resize_ksize(%d, %r, %r, %d)" % (in_size, b0, b1, out_size))
    return k


def resize_taps(in_size, b0, b1, out_size, lib=None, filter=FILTER_BILINEAR):
    """mbn_resize_taps_filter: (first [out_size], count [out_size], weights [out_size][ksize]) of one axis, int32."""
    lib = lib or host_lib()
    ks = resize_ksize(in_size, b0, b1, out_size, lib, filter)
    first, count, weights = np.zeros(out_size, np.int32), np.zeros(out_size, np.int32), np.zeros((out_size, ks), np.int32)
    i32p = C.POINTER(C.c_int32)
    rc = lib.mbn_resize_taps_filter(filter, in_size, b0, b1, out_size, first.ctypes.data_as(i32p), count.ctypes.data_as(i32p),
                                    weights.ctypes.data_as(i32p))
    if rc < 0:
        raise MbnError(rc, "resize_taps")
    return first, count, weights


def resize_nearest_index(in_size, b0, b1, out_size, lib=None) -> np.ndarray:
    """mbn_resize_nearest_index: the source position of every output of one axis under FILTER_NEAREST, int32 [out_size]."""
    index = np.zeros(out_size, np.int32)
    _chk((lib or host_lib()).mbn_resize_nearest_index(in_size, b0, b1, out_size, index.ctypes.data_as(C.POINTER(C.c_int32))), "resize_nearest_index")
    return index


def fit_box(in_rows, in_cols, out_rows, out_cols, fit=FIT_CROP, crop_fraction=1.0, lib=None) -> np.ndarray:
    """mbn_fit_box: (left, upper, right, lower) as float32 for FIT_STRETCH (the whole image) or FIT_CROP (the centred box with the output's
    aspect ratio, shrunk by crop_fraction)."""
    box = (C.c_float * 4)()
    _chk((lib or host_lib()).mbn_fit_box(in_rows, in_cols, out_rows, out_cols, fit, crop_fraction, box), "fit_box")
    return np.array(box[:], np.float32)


def fit_pad(in_rows, in_cols, out_rows, out_cols, lib=None):
    """mbn_fit_pad: (x, y, iw, ih) of the letterbox of an in_rows x in_cols image in an out_rows x out_cols canvas (PIL.ImageOps.pad, centred)."""
    rect = (C.c_int32 * 4)()
    _chk((lib or host_lib()).mbn_fit_pad(in_rows, in_cols, out_rows, out_cols, rect), "fit_pad(%d, %d, %d, %d)" % (in_rows, in_cols, out_rows, out_cols))
    return tuple(rect[:])


def fit_view(in_rows, in_cols, out_rows, out_cols, scale=1.0, mirror=0, lib=None) -> View:
    """mbn_fit_view: the view of an in_rows x in_cols image at `scale` (0 < scale <= 1) in an out_rows x out_cols network input: fit_pad into the
    canvas scaled about its centre; mirror 0 / 1 applies to the inner image alone."""
    v = View()
    _chk((lib or host_lib()).mbn_fit_view(in_rows, in_cols, out_rows, out_cols, scale, mirror, C.byref(v)),
         "fit_view(%d, %d, %d, %d, %r, %r)" % (in_rows, in_cols, out_rows, out_cols, scale, mirror))
    return v


def views(items):
    """A C array of mbn_view from View objects or (x, y, iw, ih, mirror) tuples."""
    arr = (View * len(items))()
    for dst, it in zip(arr, items):
        if isinstance(it, View):
            C.memmove(C.byref(dst), C.byref(it), C.sizeof(View))
        else:
            dst.x, dst.y, dst.iw, dst.ih, dst.mirror = (int(v) for v in it)
    return arr


def resample_ensemble_envelope(batch, rows, cols, classes, in_rows, in_cols, view_list, out_rows, out_cols, lib=None, n_views=None) -> int:
    """mbn_resample_ensemble_envelope: the status mbn_resample_ensemble_f32 gives the shape and the views (n_views: the count handed over, for the
    refusals; the list's length by default)."""
    arr = view_list if isinstance(view_list, C.Array) else views(view_list)
    return (lib or host_lib()).mbn_resample_ensemble_envelope(batch, rows, cols, classes, in_rows, in_cols, arr, len(arr) if n_views is None else n_views,
                                                              out_rows, out_cols)


def resample_ensemble_plan(rows, cols, in_rows, in_cols, view_list, out_rows, out_cols, lib=None) -> ResampleLaunch:
    """mbn_resample_ensemble_plan: the launch of a set of views: the largest footprint over them, the class chunk that keeps all of them in 64 KB."""
    arr = view_list if isinstance(view_list, C.Array) else views(view_list)
    l = ResampleLaunch()
    _chk((lib or host_lib()).mbn_resample_ensemble_plan(rows, cols, in_rows, in_cols, arr, len(arr), out_rows, out_cols, C.byref(l)),
         "resample_ensemble_plan")
    return l


def slide_axis(size, tile, stride, lib=None) -> list:
    """mbn_slide_axis: the positions of the tiles along an axis of `size`: regular steps, the last tile flush with the far edge."""
    pos, n = (C.c_int32 * SLIDE_MAX_AXIS)(), C.c_int32()
    _chk((lib or host_lib()).mbn_slide_axis(size, tile, stride, pos, C.byref(n)), "slide_axis(%d, %d, %d)" % (size, tile, stride))
    return list(pos[:n.value])


def slide_plan(in_rows, in_cols, tile_rows, tile_cols, stride_rows, stride_cols, lib=None) -> Slide:
    """mbn_slide_plan: the grid of tiles over an in_rows x in_cols image."""
    s = Slide()
    _chk((lib or host_lib()).mbn_slide_plan(in_rows, in_cols, tile_rows, tile_cols, stride_rows, stride_cols, C.byref(s)),
         "slide_plan(%d, %d, %d, %d, %d, %d)" % (in_rows, in_cols, tile_rows, tile_cols, stride_rows, stride_cols))
    return s


def slide(plan) -> Slide:
    """A Slide from a Slide or a hand-made (tile_rows, tile_cols, ys, xs)."""
    if isinstance(plan, Slide):
        return plan
    s = Slide()
    s.tile_rows, s.tile_cols, ys, xs = plan
    s.ny, s.nx = len(ys), len(xs)
    for i, v in enumerate(ys[:SLIDE_MAX_AXIS]):
        s.y[i] = int(v)
    for i, v in enumerate(xs[:SLIDE_MAX_AXIS]):
        s.x[i] = int(v)
    return s


def resample_slide_envelope(batch, rows, cols, classes, plan, out_rows, out_cols, lib=None) -> int:
    """mbn_resample_slide_envelope: the status mbn_resample_slide_f32 gives the shape and the plan (None: a NULL plan)."""
    return (lib or host_lib()).mbn_resample_slide_envelope(batch, rows, cols, classes, None if plan is None else C.byref(slide(plan)), out_rows, out_cols)


def resample_slide_plan(rows, cols, plan, out_rows, out_cols, lib=None) -> ResampleLaunch:
    """mbn_resample_slide_plan: the launch of a grid of tiles: a tile's footprint, the class chunk that keeps the most tiles over a piece in 64 KB,
    one workgroup per piece of constant coverage."""
    l = ResampleLaunch()
    _chk((lib or host_lib()).mbn_resample_slide_plan(rows, cols, C.byref(slide(plan)), out_rows, out_cols, C.byref(l)), "resample_slide_plan")
    return l


def _fill3(pad):
    """A letterbox's border colour (R, G, B) as a C uint8[3]."""
    r, g, b = (int(v) for v in pad)
    return (C.c_uint8 * 3)(r, g, b)


def resize_items(items):
    """A C array of mbn_resize_item from (src_offset, rows, cols, box) tuples; box None = the whole image."""
    arr = (ResizeItem * len(items))()
    for it, (off, rows, cols, box) in zip(arr, items):
        it.src_offset, it.rows, it.cols = int(off), int(rows), int(cols)
        it.box[:] = [float(np.float32(v)) for v in (box if box is not None else (0.0, 0.0, cols, rows))]
    return arr


def resize_window(in_size, b0, b1, out_size, o_first, o_last, lib=None, filter=FILTER_BILINEAR):
    """mbn_resize_window_filter: [lo, hi) of the source positions the outputs o_first..o_last of an axis reach (no table is built)."""
    lo, hi = C.c_int32(), C.c_int32()
    _chk((lib or host_lib()).mbn_resize_window_filter(filter, in_size, b0, b1, out_size, o_first, o_last, C.byref(lo), C.byref(hi)), "resize_window")
    return lo.value, hi.value


def resize_table_plan(in_rows, in_cols, out_rows, out_cols, box=None, lib=None, filter=FILTER_BILINEAR) -> ResizePlan:
    """mbn_resize_table_plan_filter: the tile mbn_resizer_create_filter chooses for a geometry (box None = the whole image)."""
    p = ResizePlan()
    _chk((lib or host_lib()).mbn_resize_table_plan_filter(filter, in_rows, in_cols, _box4(box), out_rows, out_cols, C.byref(p)),
         "resize_table_plan(%d, %d, %d, %d)" % (in_rows, in_cols, out_rows, out_cols))
    return p


def resize_pad_table_plan(in_rows, in_cols, out_rows, out_cols, lib=None, filter=FILTER_BILINEAR) -> ResizePadPlan:
    """mbn_resize_pad_table_plan_filter: what mbn_resizer_create_pad plans: the tile of (in_rows, in_cols) -> (ih, iw), the rectangle, the border."""
    p = ResizePadPlan()
    _chk((lib or host_lib()).mbn_resize_pad_table_plan_filter(filter, in_rows, in_cols, out_rows, out_cols, C.byref(p)),
         "resize_pad_table_plan(%d, %d, %d, %d)" % (in_rows, in_cols, out_rows, out_cols))
    return p


def resize_pad_ragged_plan(items, out_rows, out_cols, lib=None, filter=FILTER_BILINEAR):
    """mbn_resize_pad_ragged_plan_batch_filter: (descriptors, workgroups, dynamic LDS bytes, bytes of src reached) of a letterbox launch of `items`."""
    arr = items if isinstance(items, C.Array) else resize_items(items)
    desc = (ResizePadDesc * len(arr))()
    wgs, lds, span = C.c_int32(), C.c_int32(), C.c_int64()
    _chk((lib or host_lib()).mbn_resize_pad_ragged_plan_batch_filter(filter, arr, len(arr), out_rows, out_cols, desc, C.byref(wgs), C.byref(lds),
                                                                      C.byref(span)), "resize_pad_ragged_plan")
    return desc, wgs.value, lds.value, span.value


def resize_ragged_plan(items, out_rows, out_cols, lib=None, filter=FILTER_BILINEAR):
    """mbn_resize_ragged_plan_batch_filter: (descriptors, workgroups, dynamic LDS bytes, bytes of src reached) of a ragged launch of `items`
    ((src_offset, rows, cols, box) tuples, or a ResizeItem array)."""
    arr = items if isinstance(items, C.Array) else resize_items(items)
    desc = (ResizeDesc * len(arr))()
    wgs, lds, span = C.c_int32(), C.c_int32(), C.c_int64()
    _chk((lib or host_lib()).mbn_resize_ragged_plan_batch_filter(filter, arr, len(arr), out_rows, out_cols, desc, C.byref(wgs), C.byref(lds),
                                                                  C.byref(span)), "resize_ragged_plan")
    return desc, wgs.value, lds.value, span.value


def label_items(items):
    """A C array of mbn_label_item from (dst_offset, rows, cols) tuples."""
    arr = (LabelItem * len(items))()
    for it, (off, rows, cols) in zip(arr, items):
        it.dst_offset, it.rows, it.cols = int(off), int(rows), int(cols)
    return arr


def label_window_items(items):
    """A C array of mbn_label_window_item from (dst_offset, rows, cols, (x, y, iw, ih)) tuples."""
    arr = (LabelWindowItem * len(items))()
    for it, (off, rows, cols, rect) in zip(arr, items):
        it.dst_offset, it.rows, it.cols = int(off), int(rows), int(cols)
        it.x, it.y, it.iw, it.ih = (int(v) for v in rect)
    return arr


def _rect(rect):
    return (C.c_int32 * 4)(*[int(v) for v in rect])


def resample_window_envelope(batch, rows, cols, classes, in_rows, in_cols, rect, out_rows, out_cols, lib=None) -> int:
    """mbn_resample_window_envelope: the status mbn_resample_argmax_window_f32 gives the shape and the window rect = (x, y, iw, ih)."""
    return (lib or host_lib()).mbn_resample_window_envelope(batch, rows, cols, classes, in_rows, in_cols, None if rect is None else _rect(rect),
                                                            out_rows, out_cols)


def resample_window_plan(rows, cols, in_rows, in_cols, rect, out_rows, out_cols, lib=None) -> ResampleLaunch:
    """mbn_resample_window_plan: the launch of one output size of one window of a rows x cols map."""
    l = ResampleLaunch()
    (lib or host_lib()).mbn_resample_window_plan(rows, cols, in_rows, in_cols, _rect(rect), out_rows, out_cols, C.byref(l))
    return l


def resample_ragged_window_check(rows, cols, classes, in_rows, in_cols, items, launch=None, lib=None):
    """mbn_resample_ragged_window_check: (status, launch) of a ragged window set of (dst_offset, rows, cols, rect) tuples. `launch`: the record
    to write into (a refused batch leaves it as it was)."""
    arr = items if isinstance(items, C.Array) else label_window_items(items)
    l = launch if launch is not None else ResampleLaunch()
    rc = (lib or host_lib()).mbn_resample_ragged_window_check(rows, cols, classes, in_rows, in_cols, arr, len(arr),
                                                              (C.c_int64 * (2 * max(len(arr), 1)))(), C.byref(l))
    return rc, l


def softmax_readout_check(have_prob, min_prob, lib=None) -> int:
    """mbn_softmax_readout_check: the status (OK or EINVAL) the softmax read-outs give min_prob, with or without a prob map."""
    return (lib or host_lib()).mbn_softmax_readout_check(1 if have_prob else 0, min_prob)


def resample_argmax_envelope(batch, rows, cols, classes, out_rows, out_cols, lib=None) -> int:
    """mbn_resample_argmax_envelope: the status (OK, EINVAL or EUNSUPPORTED) mbn_resample_argmax_f32 gives the shape."""
    return (lib or host_lib()).mbn_resample_argmax_envelope(batch, rows, cols, classes, out_rows, out_cols)


def resample_plan(rows, cols, out_rows, out_cols, lib=None) -> ResampleLaunch:
    """mbn_resample_plan: the launch of one output size of a rows x cols map (LDS footprint, class chunk, dynamic LDS, tiles)."""
    l = ResampleLaunch()
    (lib or host_lib()).mbn_resample_plan(rows, cols, out_rows, out_cols, C.byref(l))
    return l


def resample_ragged_check(rows, cols, classes, items, lib=None):
    """mbn_resample_ragged_check: (status, launch) of a ragged set of (dst_offset, rows, cols) tuples over a rows x cols x classes map."""
    arr = items if isinstance(items, C.Array) else label_items(items)
    l = ResampleLaunch()
    rc = (lib or host_lib()).mbn_resample_ragged_check(rows, cols, classes, arr, len(arr), (C.c_int64 * (2 * max(len(arr), 1)))(), C.byref(l))
    return rc, l


CONFUSION_MAX_CLASSES = 4096
CONFUSION_FORM_LDS, CONFUSION_FORM_GLOBAL = 0, 1


def confusion_envelope(classes, truth_bytes, count, lib=None) -> int:
    """mbn_confusion_envelope: the status (OK, EINVAL or EUNSUPPORTED) mbn_confusion_i32 gives the shape."""
    return (lib or host_lib()).mbn_confusion_envelope(classes, truth_bytes, count)


def confusion_form(classes, lib=None) -> int:
    """mbn_confusion_form: CONFUSION_FORM_LDS (a workgroup counts in LDS) or CONFUSION_FORM_GLOBAL (global atomics only) for a class count."""
    return (lib or host_lib()).mbn_confusion_form(classes)


def confusion_metrics(counts, classes, lib=None):
    """mbn_confusion_metrics: (SegMetrics, iou float64 [classes], NaN for an absent class) of counts, uint64 [classes + 1][classes + 1]."""
    n = np.ascontiguousarray(counts, dtype=np.uint64)
    if n.size != (classes + 1) ** 2:
        raise ValueError("counts has %d cells, classes = %d needs %d" % (n.size, classes, (classes + 1) ** 2))
    m, iou = SegMetrics(), np.empty(classes, np.float64)
    _chk((lib or host_lib()).mbn_confusion_metrics(n.ctypes.data_as(C.POINTER(C.c_uint64)), classes, C.byref(m),
                                                   iou.ctypes.data_as(C.POINTER(C.c_double))), "confusion_metrics")
    return m, iou


TOPK_MAX = 8
TOPK_MAX_ELEMENTS = 1 << 40


def resample_topk_envelope(batch, rows, cols, classes, in_rows, in_cols, rect, out_rows, out_cols, k, lib=None) -> int:
    """mbn_resample_topk_envelope: the status mbn_resample_topk_f32 gives the shape, the window rect = (x, y, iw, ih) (None: the whole map) and k."""
    return (lib or host_lib()).mbn_resample_topk_envelope(batch, rows, cols, classes, in_rows, in_cols, None if rect is None else _rect(rect),
                                                          out_rows, out_cols, k)


def resample_topk_ragged_check(classes, span, k, plane_stride, lib=None) -> int:
    """mbn_resample_topk_ragged_check: the status mbn_resample_topk_ragged_f32 gives k and plane_stride for a set that reaches `span` elements."""
    return (lib or host_lib()).mbn_resample_topk_ragged_check(classes, span, k, plane_stride)


def topk_rank_envelope(classes, truth_bytes, count, k, plane_stride, lib=None) -> int:
    """mbn_topk_rank_envelope: the status (OK, EINVAL or EUNSUPPORTED) mbn_topk_rank_i32 gives the shape."""
    return (lib or host_lib()).mbn_topk_rank_envelope(classes, truth_bytes, count, k, plane_stride)


def topk_rank_form(classes, k, lib=None) -> int:
    """mbn_topk_rank_form: CONFUSION_FORM_LDS (a workgroup counts in LDS) or CONFUSION_FORM_GLOBAL for a table of (classes + 1) x (k + 1)."""
    return (lib or host_lib()).mbn_topk_rank_form(classes, k)


def topk_metrics(ranks, classes, k, lib=None):
    """mbn_topk_metrics: (accuracy float64 [k], mean_accuracy float64 [k], valid) of ranks, uint64 [classes + 1][k + 1]: top-1 .. top-k."""
    n = np.ascontiguousarray(ranks, dtype=np.uint64)
    if n.size != (classes + 1) * (k + 1):
        raise ValueError("ranks has %d cells, classes = %d and k = %d need %d" % (n.size, classes, k, (classes + 1) * (k + 1)))
    acc, mean, valid = np.empty(max(k, 1), np.float64), np.empty(max(k, 1), np.float64), C.c_double()
    dp = C.POINTER(C.c_double)
    _chk((lib or host_lib()).mbn_topk_metrics(n.ctypes.data_as(C.POINTER(C.c_uint64)), classes, k, acc.ctypes.data_as(dp), mean.ctypes.data_as(dp),
                                              C.byref(valid)), "topk_metrics")
    return acc, mean, valid.value


CALIBRATION_MAX_BINS = 1024
CALIBRATION_ONE = 1 << 24           # the fixed point of a table's confidence column


def calibration_envelope(classes, truth_bytes, bins, count, lib=None) -> int:
    """mbn_calibration_envelope: the status (OK, EINVAL or EUNSUPPORTED) mbn_calibration_f32 gives the shape."""
    return (lib or host_lib()).mbn_calibration_envelope(classes, truth_bytes, bins, count)


def _calibration_table(calib, bins):
    n = np.ascontiguousarray(calib, dtype=np.uint64)
    if n.size != (bins + 1) * 4:
        raise ValueError("calib has %d cells, bins = %d needs %d" % (n.size, bins, (bins + 1) * 4))
    return n


def calibration_metrics(calib, bins, lib=None):
    """mbn_calibration_metrics: (Calibration, accuracy, confidence, coverage, selective_accuracy), each array float64 [bins], of calib, uint64
    [bins + 1][4]: the reliability diagram (NaN for an empty bin), ECE / MCE, and the risk-coverage curve of keeping the bins >= j with its AURC."""
    n = _calibration_table(calib, bins)
    m, out = Calibration(), [np.empty(max(bins, 1), np.float64) for _ in range(4)]
    dp = C.POINTER(C.c_double)
    _chk((lib or host_lib()).mbn_calibration_metrics(n.ctypes.data_as(C.POINTER(C.c_uint64)), bins, C.byref(m),
                                                     *[a.ctypes.data_as(dp) for a in out]), "calibration_metrics")
    return (m, *out)


def calibration_threshold(calib, bins, target_accuracy, lib=None):
    """mbn_calibration_threshold: (min_prob, coverage, selective_accuracy) of the smallest edge j / bins whose kept pixels reach target_accuracy;
    None when no edge does (MBN_ENOTFOUND)."""
    n = _calibration_table(calib, bins)
    p, cov, sel = C.c_float(), C.c_double(), C.c_double()
    rc = (lib or host_lib()).mbn_calibration_threshold(n.ctypes.data_as(C.POINTER(C.c_uint64)), bins, target_accuracy, C.byref(p), C.byref(cov),
                                                       C.byref(sel))
    if rc == ENOTFOUND:
        return None
    _chk(rc, "calibration_threshold")
    return p.value, cov.value, sel.value


NLL_MAX_TEMPS = 8
NLL_CAP = 32768.0
NLL_ONE = 1 << 16                   # the fixed point of a table's NLL column (the Brier column: CALIBRATION_ONE)


def _inv_temps(inv_temps):
    """a host array of fp32 inverse temperatures as ctypes, and its length"""
    v = [float(b) for b in inv_temps]
    return (C.c_float * max(len(v), 1))(*v), len(v)


def nll_envelope(batch, rows, cols, classes, in_rows, in_cols, rect, out_rows, out_cols, truth_bytes, temps, lib=None) -> int:
    """mbn_resample_nll_envelope: the status mbn_resample_nll_f32 gives the shape, the window rect (None: the whole map), the truth and temps."""
    return (lib or host_lib()).mbn_resample_nll_envelope(batch, rows, cols, classes, in_rows, in_cols, None if rect is None else _rect(rect),
                                                         out_rows, out_cols, truth_bytes, temps)


def _nll_table(table, classes, temps):
    n = np.ascontiguousarray(table, dtype=np.uint64)
    if n.size != temps * (classes + 1) * 4:
        raise ValueError("the table has %d cells, classes = %d and temps = %d need %d" % (n.size, classes, temps, temps * (classes + 1) * 4))
    return n


def nll_metrics(table, classes, temps, j, lib=None):
    """mbn_nll_metrics: (Nll, class_nll float64 [classes], class_brier float64 [classes]) of plane j of table, uint64 [temps][classes + 1][4]."""
    n = _nll_table(table, classes, temps)
    m, cn, cb = Nll(), np.empty(max(classes, 1), np.float64), np.empty(max(classes, 1), np.float64)
    dp = C.POINTER(C.c_double)
    _chk((lib or host_lib()).mbn_nll_metrics(n.ctypes.data_as(C.POINTER(C.c_uint64)), classes, temps, j, C.byref(m), cn.ctypes.data_as(dp),
                                             cb.ctypes.data_as(dp)), "nll_metrics")
    return m, cn, cb


def nll_best(table, classes, inv_temps, lib=None):
    """mbn_nll_best: (best index, refined inverse temperature, at_edge) of a table over the strictly ascending grid inv_temps; None when nothing
    is scored (MBN_ENOTFOUND)."""
    arr, temps = _inv_temps(inv_temps)
    n = _nll_table(table, classes, temps)
    best, beta, edge = C.c_int(), C.c_double(), C.c_int()
    rc = (lib or host_lib()).mbn_nll_best(n.ctypes.data_as(C.POINTER(C.c_uint64)), classes, temps, arr, C.byref(best), C.byref(beta), C.byref(edge))
    if rc == ENOTFOUND:
        return None
    _chk(rc, "nll_best")
    return best.value, beta.value, edge.value


COMPONENTS_MAX_REGIONS = 1 << 24


def components_envelope(batch, rows, cols, classes, connectivity=4, min_area=1, max_regions=0, lib=None) -> int:
    """mbn_components_envelope: the status (OK, EINVAL or EUNSUPPORTED) mbn_components_i32 gives the shape."""
    return (lib or host_lib()).mbn_components_envelope(batch, rows, cols, classes, connectivity, min_area, max_regions)


def components_tile(lib=None):
    """mbn_components_tile: (tile_rows, tile_cols) of the first kernel: a seam of the union-find lies at every multiple of them."""
    tr, tc = C.c_int(), C.c_int()
    _chk((lib or host_lib()).mbn_components_tile(C.byref(tr), C.byref(tc)), "components_tile")
    return tr.value, tc.value


BOUNDARY_MAX_D = 64


def boundary_d(rows, cols, ratio, lib=None) -> int:
    """mbn_boundary_d: the half-width round (ratio * diagonal), ties to even, at least 1; or the negative status (EINVAL, EUNSUPPORTED)."""
    return (lib or host_lib()).mbn_boundary_d(rows, cols, ratio)


def boundary_envelope(elem_bytes, classes, batch, rows, cols, d, edge, lib=None) -> int:
    """mbn_boundary_envelope: the status (OK, EINVAL or EUNSUPPORTED) the boundary calls give the shape (classes = 1 for the depth calls)."""
    return (lib or host_lib()).mbn_boundary_envelope(elem_bytes, classes, batch, rows, cols, d, edge)


def boundary_tile(d, lib=None):
    """mbn_boundary_tile: (tile_rows, tile_cols, lds_bytes) of the kernel at half-width d: a seam lies at every multiple of the tile."""
    tr, tc, lds = C.c_int(0), C.c_int(0), C.c_int(0)
    _chk((lib or host_lib()).mbn_boundary_tile(d, C.byref(tr), C.byref(tc), C.byref(lds)), "boundary_tile")
    return tr.value, tc.value, lds.value


def boundary_metrics(biou, classes, lib=None):
    """mbn_boundary_metrics: (BoundaryMetrics, iou float64 [classes], NaN for an absent class) of biou, uint64 [classes][3]."""
    n = np.ascontiguousarray(biou, dtype=np.uint64)
    if n.size != classes * 3:
        raise ValueError("biou has %d cells, classes = %d needs %d" % (n.size, classes, classes * 3))
    m, iou = BoundaryMetrics(), np.empty(classes, np.float64)
    _chk((lib or host_lib()).mbn_boundary_metrics(n.ctypes.data_as(C.POINTER(C.c_uint64)), classes, C.byref(m),
                                                  iou.ctypes.data_as(C.POINTER(C.c_double))), "boundary_metrics")
    return m, iou


SURFACE_HEAD = 4                 # MBN_SURFACE_HEAD: n, unmatched, max_d2, sum256 in front of the bins of a surface table's row
SURFACE_MAX_BINS = 4096          # MBN_SURFACE_MAX_BINS
SURFACE_UNMATCHED = 0xFFFFFFFE   # dist2 of a query whose class has no contour in the other map
SURFACE_NOT_QUERY = 0xFFFFFFFF   # dist2 of a pixel that is no query


def surface_envelope(truth_bytes, classes, bins, batch, rows, cols, edge, lib=None) -> int:
    """mbn_surface_envelope: the status (OK, EINVAL or EUNSUPPORTED) the surface calls give the shape."""
    return (lib or host_lib()).mbn_surface_envelope(truth_bytes, classes, bins, batch, rows, cols, edge)


def surface_tile(lib=None):
    """mbn_surface_tile: (unit_pixels, wave_pixels): a seam of the kernels lies at every multiple of them in a map's row-major pixel order."""
    up, wp = C.c_int(0), C.c_int(0)
    _chk((lib or host_lib()).mbn_surface_tile(C.byref(up), C.byref(wp)), "surface_tile")
    return up.value, wp.value


def surface_scratch_bytes(max_batch, max_pixels, max_classes, lib=None) -> int:
    """mbn_surface_scratch_bytes: the device memory a Surface handle of that size holds (0: a size mbn_surface_create refuses)."""
    return (lib or host_lib()).mbn_surface_scratch_bytes(max_batch, max_pixels, max_classes)


def surface_metrics(surf, classes, bins, tolerance=2, percentile=95.0, lib=None):
    """mbn_surface_metrics: (SurfaceMetrics, hd, hdp, assd, nsd: float64 [classes], NaN where a score is undefined) of surf, uint64
    [classes][2][SURFACE_HEAD + bins]. A micro average: the table pools the contour pixels of every image and call."""
    n = np.ascontiguousarray(surf, dtype=np.uint64)
    if n.size != classes * 2 * (SURFACE_HEAD + bins):
        raise ValueError("surf has %d cells, classes = %d and bins = %d need %d" % (n.size, classes, bins, classes * 2 * (SURFACE_HEAD + bins)))
    m, out = SurfaceMetrics(), [np.empty(classes, np.float64) for _ in range(4)]
    _chk((lib or host_lib()).mbn_surface_metrics(n.ctypes.data_as(C.POINTER(C.c_uint64)), classes, bins, tolerance, percentile, C.byref(m),
                                                 *[o.ctypes.data_as(C.POINTER(C.c_double)) for o in out]), "surface_metrics")
    return (m,) + tuple(out)


PANOPTIC_CHUNK = 1024            # MBN_PANOPTIC_CHUNK: the pixels of one unit of work of the two pixel kernels of mbn_panoptic_i32
PANOPTIC_LDS_CLASSES = 1024      # MBN_PANOPTIC_LDS_CLASSES: up to here its two deciding kernels count a workgroup's classes in LDS
NET_PANOPTIC_REGIONS = 4096      # MBN_NET_PANOPTIC_REGIONS


def panoptic_envelope(batch, rows, cols, classes, max_pred, max_truth, lib=None) -> int:
    """mbn_panoptic_envelope: the status (OK, EINVAL or EUNSUPPORTED) mbn_panoptic_i32 gives the shape."""
    return (lib or host_lib()).mbn_panoptic_envelope(batch, rows, cols, classes, max_pred, max_truth)


def panoptic_scratch_bytes(max_batch, max_slots, lib=None) -> int:
    """mbn_panoptic_scratch_bytes: the device memory a Panoptic handle of that size holds (0: a size mbn_panoptic_create refuses)."""
    return (lib or host_lib()).mbn_panoptic_scratch_bytes(max_batch, max_slots)


def panoptic_metrics(pq, classes, lib=None):
    """mbn_panoptic_metrics: (PanopticMetrics, pq_c, sq_c, rq_c: float64 [classes], NaN for an absent class) of pq, uint64 [classes][4] =
    tp, fp, fn, S."""
    n = np.ascontiguousarray(pq, dtype=np.uint64)
    if n.size != classes * 4:
        raise ValueError("pq has %d cells, classes = %d needs %d" % (n.size, classes, classes * 4))
    m, out = PanopticMetrics(), [np.empty(classes, np.float64) for _ in range(3)]
    _chk((lib or host_lib()).mbn_panoptic_metrics(n.ctypes.data_as(C.POINTER(C.c_uint64)), classes, C.byref(m),
                                                  *[o.ctypes.data_as(C.POINTER(C.c_double)) for o in out]), "panoptic_metrics")
    return (m,) + tuple(out)


def components_scratch_bytes(max_batch, max_pixels, lib=None) -> int:
    """mbn_components_scratch_bytes: the device memory a Components handle of that size holds (0: a size mbn_components_create refuses)."""
    return (lib or host_lib()).mbn_components_scratch_bytes(max_batch, max_pixels)


def declared_symbols():
    """Every function name declared in include/mbn.h (for the export test)."""
    import re
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = re.findall(r"\b((?:mbn_[a-z0-9_]+)|readSquezeNetKernel|decode_image)\s*\(", src)
    return sorted(set(n for n in names if n not in ("mbn_layer_ext", "mbn_context")))


def make_ext(batch=1, dtype=DT_F32, act=ACT_RELU6, pad_top=-1, pad_left=-1, in_rows=0, in_cols=0, cin=0, scale=None,
             shift=None, quirks=None, gsize=(0, 0), stream=None, io_flags=0, dilation=0) -> LayerExt:
    e = LayerExt()
    e.struct_size = C.sizeof(LayerExt)
    e.batch = batch
    e.dtype = dtype
    e.layout = LAYOUT_NCHW_PLANAR if dtype == DT_U8 else LAYOUT_NHWC
    e.io_flags = io_flags
    e.act = act
    e.pad_top, e.pad_left = pad_top, pad_left
    e.in_rows, e.in_cols, e.cin = in_rows, in_cols, cin
    e.dilation = dilation                 # depthwise only: 0 / 1 = none
    e.gsize0, e.gsize1 = gsize
    if quirks is not None:
        e.quirks, e.quirks_valid = quirks, 1
    e.scale = scale
    e.shift = shift
    e.stream = stream
    return e


def bf16_bits_to_f32(raw: np.ndarray) -> np.ndarray:
    """uint16 bf16 bit patterns -> float32 values."""
    return (raw.astype(np.uint32) << 16).view(np.float32)


def f32_to_bf16_bits(x: np.ndarray) -> np.ndarray:
    """float32 -> bf16 bit patterns, round to nearest even (host-side helper for tests)."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def packed_filter_dev(ctx, filt_f32: np.ndarray):
    """Device buffer holding a bf16 pointwise filter [cout][cin] followed by its packed image (mbn_pack_filter_bf16), for calls with
    IO_FILT_PACKED; when the shape has no packed form the buffer holds the plain filter only. Returns (buffer, io_flag)."""
    cout, cin = filt_f32.shape
    off = ctx.lib.mbn_packed_filter_offset(cout, cin)
    bits = f32_to_bf16_bits(filt_f32)
    buf = ctx.alloc(off + bits.nbytes if off else bits.nbytes)
    buf.upload(bits)
    if off:
        _chk(ctx.lib.mbn_pack_filter_bf16(ctx.h, buf.ptr, cout, cin, None), ctx.last_error())
        ctx.sync()
    return buf, (IO_FILT_PACKED if off else 0)


class DeviceBuffer:
    """A device allocation owned by a Context (mbn_alloc / mbn_free)."""

    def __init__(self, ctx: "Context", nbytes: int):
        self.ctx, self.nbytes = ctx, int(nbytes)
        p = C.c_void_p()
        _chk(ctx.lib.mbn_alloc(ctx.h, max(self.nbytes, 1), C.byref(p)), "alloc %d" % nbytes)
        self.ptr = p.value

    def upload(self, arr: np.ndarray):
        a = np.ascontiguousarray(arr)
        assert a.nbytes <= self.nbytes
        _chk(self.ctx.lib.mbn_upload(self.ctx.h, self.ptr, a.ctypes.data, a.nbytes))
        return self

    def download(self, shape, dtype) -> np.ndarray:
        out = np.empty(shape, dtype)
        assert out.nbytes <= self.nbytes
        _chk(self.ctx.lib.mbn_download(self.ctx.h, out.ctypes.data, self.ptr, out.nbytes))
        return out

    def free(self):
        if self.ptr:
            self.ctx.lib.mbn_free(self.ctx.h, self.ptr)
            self.ptr = None


class Context:
    """mbn_init / mbn_shutdown. Raises MbnError(ENODEVICE) when no MI355X is visible."""

    def __init__(self, device: int = 0):
        self.lib = load()
        h = C.c_void_p()
        _chk(self.lib.mbn_init(device, C.byref(h)), "mbn_init(%d)" % device)
        self.h = h
        self._bufs = []

    def name(self) -> str:
        b = C.create_string_buffer(128)
        self.lib.mbn_device_name(self.h, b, 128)
        return b.value.decode()

    def pci_bus_id(self) -> str:
        b = C.create_string_buffer(64)
        _chk(self.lib.mbn_device_pci_bus_id(self.h, b, 64), self.last_error())
        return b.value.decode()

    def device_cus(self) -> int:
        """mbn_device_cus: the count the launches are planned for (the device's own unless set_planning_cus changed it)."""
        n = C.c_int()
        _chk(self.lib.mbn_device_cus(self.h, C.byref(n)), "mbn_device_cus")
        return n.value

    def set_planning_cus(self, cus: int):
        """mbn_set_planning_cus: plan every launch for `cus` compute units (0 = the device's own count). Not while launches are in flight."""
        _chk(self.lib.mbn_set_planning_cus(self.h, int(cus)), "mbn_set_planning_cus(%d)" % cus)

    def pw_clock(self, reset=True):
        """(GHz, launches): the core clock held inside the pw_gemm launches recorded since the last reset (tune key pw_clock)."""
        g, n = C.c_double(), C.c_longlong()
        _chk(self.lib.mbn_pw_clock_read(self.h, int(reset), C.byref(g), C.byref(n)), self.last_error())
        return g.value, n.value

    def alloc(self, nbytes) -> DeviceBuffer:
        b = DeviceBuffer(self, nbytes)
        self._bufs.append(b)
        return b

    def to_device(self, arr: np.ndarray) -> DeviceBuffer:
        a = np.ascontiguousarray(arr)
        return self.alloc(a.nbytes).upload(a)

    def sync(self):
        _chk(self.lib.mbn_sync(self.h), self.last_error())

    def last_error(self) -> str:
        return self.lib.mbn_last_device_error(self.h).decode()

    def stream(self) -> int:
        s = C.c_void_p()
        _chk(self.lib.mbn_get_stream(self.h, C.byref(s)))
        return s.value or 0

    def profile_begin(self, capacity: int):
        _chk(self.lib.mbn_profile_begin(self.h, capacity))

    def profile_pause(self, paused: bool):
        _chk(self.lib.mbn_profile_pause(self.h, int(paused)))

    def profile_end(self, capacity: int):
        ms = (C.c_float * capacity)()
        n = C.c_int()
        _chk(self.lib.mbn_profile_end(self.h, ms, capacity, C.byref(n)), self.last_error())
        return [ms[i] for i in range(n.value)]

    def profile_null_us(self, with_kernel: bool, n: int = 200) -> float:
        """Median reading (microseconds) of an event pair recorded around nothing / around an empty kernel (mbn_profile_null)."""
        self.profile_begin(n)
        for _ in range(n):
            _chk(self.lib.mbn_profile_null(self.h, int(with_kernel), None))
        ms = sorted(self.profile_end(n))
        return 1000.0 * ms[len(ms) // 2]

    def mark(self, stream=None):
        _chk(self.lib.mbn_mark(self.h, stream))

    def marks_read(self, capacity: int):
        ms = (C.c_float * max(capacity, 1))()
        n = C.c_int()
        _chk(self.lib.mbn_marks_read(self.h, ms, capacity, C.byref(n)), self.last_error())
        return [ms[i] for i in range(n.value)]

    def close(self):
        if self.h:
            self.lib.mbn_shutdown(self.h)          # frees the resizers still alive as well: their handles are dead from here on
            self.h = None
            for r in getattr(self, "_resizers", []):
                r.h = None

    # ---- layer calls: positional arguments are kernel.cl's ----
    def convolute(self, out, inp_r, inp_g, inp_b, filt, rows, cols, filtersize, stride, op_size, ext=None):
        _chk(self.lib.mbn_convolute(self.h, out, inp_r, inp_g, inp_b, filt, rows, cols, filtersize, stride, op_size,
                                    None if ext is None else C.byref(ext)), self.last_error())

    def depthwise(self, out, inp, filt, rows, cols, filtersize, stride, op_size, ext=None):
        _chk(self.lib.mbn_depthwise(self.h, out, inp, filt, rows, cols, filtersize, stride, op_size,
                                    None if ext is None else C.byref(ext)), self.last_error())

    def pointwise(self, out, inp, filt, rows, cols, filtersize, op_size, ext=None):
        _chk(self.lib.mbn_pointwise(self.h, out, inp, filt, rows, cols, filtersize, op_size,
                                    None if ext is None else C.byref(ext)), self.last_error())

    def pool(self, out, inp, rows, cols, filtersize, op_size, ext=None):
        _chk(self.lib.mbn_pool(self.h, out, inp, rows, cols, filtersize, op_size,
                               None if ext is None else C.byref(ext)), self.last_error())

    def upsample_argmax(self, labels, score, logits, batch, rows, cols, classes, factor):
        """mbn_upsample_argmax_f32: fp32 logits [batch][rows][cols][classes] -> int32 labels (and, unless `score` is None, the winning fp32
        logit) [batch][rows*factor][cols*factor]: bilinear upsample + argmax in one kernel."""
        _chk(self.lib.mbn_upsample_argmax_f32(self.h, labels, score, logits, batch, rows, cols, classes, factor, None), self.last_error())

    def resample_argmax(self, labels, score, logits, batch, rows, cols, classes, out_rows, out_cols):
        """mbn_resample_argmax_f32: fp32 logits [batch][rows][cols][classes] -> int32 labels (and, unless `score` is None, the winning fp32
        logit) [batch][out_rows][out_cols]: bilinear resample to any size (at least 4 x the map) + argmax in one kernel."""
        _chk(self.lib.mbn_resample_argmax_f32(self.h, labels, score, logits, batch, rows, cols, classes, out_rows, out_cols, None), self.last_error())

    def resample_argmax_window(self, labels, score, logits, batch, rows, cols, classes, in_rows, in_cols, rect, out_rows, out_cols):
        """mbn_resample_argmax_window_f32: the same read-out of the window rect = (x, y, iw, ih) of the in_rows x in_cols network input that the
        rows x cols map covers (fit_pad's rectangle: the labels of a letterboxed image at its own size)."""
        _chk(self.lib.mbn_resample_argmax_window_f32(self.h, labels, score, logits, batch, rows, cols, classes, in_rows, in_cols, _rect(rect),
                                                     out_rows, out_cols, None), self.last_error())

    def resample_softmax(self, labels, prob, score, logits, batch, rows, cols, classes, out_rows, out_cols, min_prob=0.0, ignore_label=0):
        """mbn_resample_softmax_f32: resample_argmax which also writes the softmax probability of the winning class (fp32 `prob`, the shape of the
        labels; None only with min_prob > 0) and stores ignore_label where that probability is below min_prob. `score` may be None."""
        _chk(self.lib.mbn_resample_softmax_f32(self.h, labels, prob, score, logits, batch, rows, cols, classes, out_rows, out_cols, min_prob,
                                               ignore_label, None), self.last_error())

    def resample_softmax_window(self, labels, prob, score, logits, batch, rows, cols, classes, in_rows, in_cols, rect, out_rows, out_cols,
                                min_prob=0.0, ignore_label=0):
        """mbn_resample_softmax_window_f32: resample_argmax_window with the probability map and the threshold of resample_softmax."""
        _chk(self.lib.mbn_resample_softmax_window_f32(self.h, labels, prob, score, logits, batch, rows, cols, classes, in_rows, in_cols, _rect(rect),
                                                      out_rows, out_cols, min_prob, ignore_label, None), self.last_error())

    def resample_ensemble(self, labels, prob, score, logits, batch, rows, cols, classes, in_rows, in_cols, view_list, out_rows, out_cols,
                          min_prob=0.0, ignore_label=0, n_views=None):
        """mbn_resample_ensemble_f32: ONE read-out of the views in view_list (View objects or (x, y, iw, ih, mirror)) over view-major logits
        [n_views][batch][rows][cols][classes]: the interpolated logits are averaged over the views in front of the argmax (and the softmax).
        prob None with min_prob 0: the argmax form. `score` may be None."""
        arr = view_list if isinstance(view_list, C.Array) else views(view_list)
        _chk(self.lib.mbn_resample_ensemble_f32(self.h, labels, prob, score, logits, batch, rows, cols, classes, in_rows, in_cols, arr,
                                                len(arr) if n_views is None else n_views, out_rows, out_cols, min_prob, ignore_label, None),
             self.last_error())

    def resample_slide(self, labels, prob, score, logits, batch, rows, cols, classes, plan, out_rows, out_cols, min_prob=0.0, ignore_label=0,
                       stream=None):
        """mbn_resample_slide_f32: ONE read-out of the grid of tiles in `plan` (a Slide or (tile_rows, tile_cols, ys, xs)) over image-major logits
        [batch][ny * nx][rows][cols][classes]: the interpolated logits are averaged over the tiles that cover a pixel in front of the argmax (and
        the softmax). prob None with min_prob 0: the argmax form. `score` may be None."""
        _chk(self.lib.mbn_resample_slide_f32(self.h, labels, prob, score, logits, batch, rows, cols, classes, C.byref(slide(plan)), out_rows, out_cols,
                                             min_prob, ignore_label, stream), self.last_error())

    def resample_topk(self, labels, prob, score, logits, batch, rows, cols, classes, out_rows, out_cols, k, rect=None, in_rows=0, in_cols=0,
                      min_prob=0.0, ignore_label=0, stream=None):
        """mbn_resample_topk_f32: the k best classes of every output pixel, rank-major: labels (int32), prob and score (fp32) are
        [k][batch][out_rows][out_cols], plane 0 the map of resample_softmax. rect = (x, y, iw, ih) of the in_rows x in_cols input, None: the whole
        map. prob None with min_prob 0: the logit form. `score` may be None. min_prob / ignore_label act on plane 0 only."""
        _chk(self.lib.mbn_resample_topk_f32(self.h, labels, prob, score, logits, batch, rows, cols, classes, in_rows, in_cols,
                                            None if rect is None else _rect(rect), out_rows, out_cols, k, min_prob, ignore_label, stream),
             self.last_error())

    def resample_nll(self, table, nll, brier, logits, truth, truth_bytes, batch, rows, cols, classes, out_rows, out_cols, inv_temps, rect=None,
                     in_rows=0, in_cols=0, stream=None):
        """mbn_resample_nll_f32: table (uint64 [temps][classes + 1][4], device) += per truth class and inverse temperature the pixels, their NLL in
        2^-16 and Brier score in 2^-24 fixed point and the pixels labelled correctly; nll / brier (fp32 [temps][batch][out_rows][out_cols], either
        may be None) get the per-pixel values, -1 on void pixels. truth (uint8 or int32) is [batch][out_rows][out_cols]; inv_temps a host list."""
        arr, temps = _inv_temps(inv_temps)
        _chk(self.lib.mbn_resample_nll_f32(self.h, table, nll, brier, logits, truth, truth_bytes, batch, rows, cols, classes, in_rows, in_cols,
                                           None if rect is None else _rect(rect), out_rows, out_cols, arr, temps, stream), self.last_error())

    def resample_nll_ragged(self, readout, table, nll, brier, plane_stride, logits, truth, truth_bytes, inv_temps, stream=None):
        """mbn_resample_nll_ragged_f32: the same over the maps of a RaggedReadout's set; temperature j of item i at j * plane_stride + dst_offset_i
        elements of nll / brier, truth at the items' element offsets."""
        arr, temps = _inv_temps(inv_temps)
        _chk(self.lib.mbn_resample_nll_ragged_f32(readout.h, table, nll, brier, plane_stride, logits, truth, truth_bytes, arr, temps, stream),
             self.last_error())

    def topk_rank(self, ranks, labels, k, plane_stride, truth, truth_bytes, classes, count, stream=None):
        """mbn_topk_rank_i32: ranks (uint64 [classes + 1][k + 1], device) += per truth row the rank at which the truth is among the k label planes
        (plane j at labels + j * plane_stride elements); column k: in none of them, and every void pixel."""
        _chk(self.lib.mbn_topk_rank_i32(self.h, ranks, labels, k, plane_stride, truth, truth_bytes, classes, count, stream), self.last_error())

    def topk_rank_ragged(self, readout, ranks, labels, k, plane_stride, truth, truth_bytes, classes, stream=None):
        """mbn_topk_rank_ragged_i32: the same over the maps of a RaggedReadout's set; truth at the labels' element offsets."""
        _chk(self.lib.mbn_topk_rank_ragged_i32(readout.h, ranks, labels, k, plane_stride, truth, truth_bytes, classes, stream), self.last_error())

    def calibration(self, calib, labels, prob, truth, truth_bytes, classes, bins, count, stream=None):
        """mbn_calibration_f32: calib (uint64 [bins + 1][4], device) += per probability bin the pixels answered, answered correctly, their
        probabilities in 2^-24 fixed point and the pixels abstained, of `count` int32 labels and fp32 probabilities against truth (uint8 or int32)."""
        _chk(self.lib.mbn_calibration_f32(self.h, calib, labels, prob, truth, truth_bytes, classes, bins, count, stream), self.last_error())

    def calibration_ragged(self, readout, calib, labels, prob, truth, truth_bytes, classes, bins, stream=None):
        """mbn_calibration_ragged_f32: the same over the maps of a RaggedReadout's set; prob and truth at the labels' element offsets."""
        _chk(self.lib.mbn_calibration_ragged_f32(readout.h, calib, labels, prob, truth, truth_bytes, classes, bins, stream), self.last_error())

    def confusion(self, counts, labels, truth, truth_bytes, classes, count, stream=None):
        """mbn_confusion_i32: counts (uint64 [classes + 1][classes + 1], device) += the confusion matrix of `count` int32 labels against truth
        (uint8: truth_bytes 1, int32: 4); row = truth (row `classes`: void), column = label (column `classes`: abstained)."""
        _chk(self.lib.mbn_confusion_i32(self.h, counts, labels, truth, truth_bytes, classes, count, stream), self.last_error())

    def confusion_ragged(self, readout, counts, labels, truth, truth_bytes, classes, stream=None):
        """mbn_confusion_ragged_i32: the same over the maps of a RaggedReadout's set; truth at the labels' element offsets."""
        _chk(self.lib.mbn_confusion_ragged_i32(readout.h, counts, labels, truth, truth_bytes, classes, stream), self.last_error())

    def components(self, handle, labels, batch, rows, cols, classes, n_regions, comp=None, regions=None, labels_out=None, connectivity=4,
                   min_area=1, ignore_label=0, max_regions=0, stream=None):
        """mbn_components_i32: the regions of int32 maps [batch][rows][cols] (device pointers): comp (region number per pixel, -1: none),
        regions (Region [batch][max_regions]), n_regions (int32 [batch], the true counts), labels_out (the maps without the dropped regions)."""
        _chk(self.lib.mbn_components_i32(handle.h, comp, regions, n_regions, labels_out, labels, batch, rows, cols, classes, connectivity, min_area,
                                         ignore_label, max_regions, stream), self.last_error())

    def boundary_depth(self, depth, map_ptr, elem_bytes, batch, rows, cols, d, edge=1, stream=None):
        """mbn_boundary_depth: depth (uint8 [batch][rows][cols], device) = min (D, d + 1) of the maps (uint8: elem_bytes 1, int32: 4)."""
        _chk(self.lib.mbn_boundary_depth(self.h, depth, map_ptr, elem_bytes, batch, rows, cols, d, edge, stream), self.last_error())

    def boundary_depth_ragged(self, readout, depth, map_ptr, elem_bytes, d, d_items=None, edge=1, stream=None):
        """mbn_boundary_depth_ragged: the same over the maps of a RaggedReadout's set; d_items: device int32 [set batch] or None (d for all)."""
        _chk(self.lib.mbn_boundary_depth_ragged(readout.h, depth, map_ptr, elem_bytes, d, d_items, edge, stream), self.last_error())

    def boundary_score(self, trimap, biou, labels, truth, truth_bytes, classes, batch, rows, cols, d, edge=1, stream=None):
        """mbn_boundary_score_i32: trimap (uint64 [classes + 1][classes + 1]) and biou (uint64 [classes][3]) += the boundary score of int32 labels
        against truth [batch][rows][cols]; either table may be None."""
        _chk(self.lib.mbn_boundary_score_i32(self.h, trimap, biou, labels, truth, truth_bytes, classes, batch, rows, cols, d, edge, stream),
             self.last_error())

    def boundary_score_ragged(self, readout, trimap, biou, labels, truth, truth_bytes, classes, d, d_items=None, edge=1, stream=None):
        """mbn_boundary_score_ragged_i32: the same over the maps of a RaggedReadout's set; truth at the labels' element offsets."""
        _chk(self.lib.mbn_boundary_score_ragged_i32(readout.h, trimap, biou, labels, truth, truth_bytes, classes, d, d_items, edge, stream),
             self.last_error())

    def boundary_d_items(self, readout, ratio):
        """mbn_boundary_d_items: int32 [set batch] (numpy), each item's own half-width at `ratio`."""
        out = np.zeros(max(readout.batch, 1), np.int32)
        _chk(self.lib.mbn_boundary_d_items(readout.h, ratio, out.ctypes.data_as(C.POINTER(C.c_int32))), self.last_error())
        return out

    def components_ragged(self, handle, readout, labels, classes, n_regions, comp=None, regions=None, labels_out=None, connectivity=4, min_area=1,
                          ignore_label=0, max_regions=0, stream=None):
        """mbn_components_ragged_i32: the same over the maps of a RaggedReadout's set; comp and labels_out at the labels' element offsets."""
        _chk(self.lib.mbn_components_ragged_i32(handle.h, readout.h, comp, regions, n_regions, labels_out, labels, classes, connectivity, min_area,
                                                ignore_label, max_regions, stream), self.last_error())

    def panoptic(self, handle, pq, scored, comp_pred, pred, n_pred, max_pred, comp_truth, truth, n_truth, max_truth, batch, rows, cols, classes,
                 match_pred=None, match_truth=None, inter=None, void=None, stream=None):
        """mbn_panoptic_i32: pq (uint64 [classes][4] = tp, fp, fn, S; device) += the panoptic score of the predicted segment maps comp_pred
        [batch][rows][cols] with their records pred (Region [batch][max_pred]) and counts n_pred (int32 [batch]) against the truth's; scored
        (int32 [batch]): 0 for an image whose tables were too small, which adds nothing."""
        _chk(self.lib.mbn_panoptic_i32(handle.h, pq, scored, match_pred, match_truth, inter, void, comp_pred, pred, n_pred, max_pred, comp_truth,
                                       truth, n_truth, max_truth, batch, rows, cols, classes, stream), self.last_error())

    def panoptic_ragged(self, handle, readout, pq, scored, comp_pred, pred, n_pred, max_pred, comp_truth, truth, n_truth, max_truth, classes,
                        match_pred=None, match_truth=None, inter=None, void=None, stream=None):
        """mbn_panoptic_ragged_i32: the same over the maps of a RaggedReadout's set; both maps at the labels' element offsets."""
        _chk(self.lib.mbn_panoptic_ragged_i32(handle.h, readout.h, pq, scored, match_pred, match_truth, inter, void, comp_pred, pred, n_pred,
                                              max_pred, comp_truth, truth, n_truth, max_truth, classes, stream), self.last_error())

    def surface_score(self, handle, surf, labels, truth, truth_bytes, classes, bins, batch, rows, cols, edge=1, dist2=None, stream=None):
        """mbn_surface_score_i32: surf (uint64 [classes][2][SURFACE_HEAD + bins], device) += the surface-distance table of int32 labels against
        truth (uint8 or int32), both [batch][rows][cols]; dist2 (uint32 at the labels' offsets, direction 0) or None."""
        _chk(self.lib.mbn_surface_score_i32(handle.h, surf, dist2, labels, truth, truth_bytes, classes, bins, batch, rows, cols, edge, stream),
             self.last_error())

    def surface_score_ragged(self, handle, readout, surf, labels, truth, truth_bytes, classes, bins, edge=1, dist2=None, stream=None):
        """mbn_surface_score_ragged_i32: the same over the maps of a RaggedReadout's set; truth and dist2 at the labels' element offsets."""
        _chk(self.lib.mbn_surface_score_ragged_i32(handle.h, readout.h, surf, dist2, labels, truth, truth_bytes, classes, bins, edge, stream),
             self.last_error())

    def widen_u8(self, dst, src, count, stream=None):
        """mbn_widen_u8_i32: dst (int32 [count]) = src (uint8 [count]), value for value."""
        _chk(self.lib.mbn_widen_u8_i32(self.h, dst, src, count, stream), self.last_error())

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class Panoptic:
    """mbn_panoptic_create: the scratch of the panoptic kernels for up to max_batch images and max_slots = batch * max (max_pred, max_truth) table
    entries in all, allocated once; the `handle` of Context.panoptic / panoptic_ragged."""

    def __init__(self, ctx: "Context", max_batch, max_slots):
        self.ctx = ctx
        h = C.c_void_p()
        _chk(ctx.lib.mbn_panoptic_create(ctx.h, max_batch, max_slots, C.byref(h)), ctx.last_error())
        self.h = h
        if not hasattr(ctx, "_resizers"):
            ctx._resizers = []
        ctx._resizers.append(self)

    def close(self):
        if self.h:
            self.ctx.lib.mbn_panoptic_destroy(self.h)
            self.h = None


class Surface:
    """mbn_surface_create: the scratch of the surface-distance kernels for up to max_batch maps of max_pixels pixels in all and max_classes classes,
    allocated once; the `handle` of Context.surface_score / surface_score_ragged."""

    def __init__(self, ctx: "Context", max_batch, max_pixels, max_classes):
        self.ctx = ctx
        h = C.c_void_p()
        _chk(ctx.lib.mbn_surface_create(ctx.h, max_batch, max_pixels, max_classes, C.byref(h)), ctx.last_error())
        self.h = h
        if not hasattr(ctx, "_resizers"):
            ctx._resizers = []
        ctx._resizers.append(self)

    def close(self):
        if self.h:
            self.ctx.lib.mbn_surface_destroy(self.h)
            self.h = None


class Components:
    """mbn_components_create: the scratch of the connected-component kernels for up to max_batch maps of max_pixels pixels in all, allocated once;
    the `handle` of Context.components / components_ragged."""

    def __init__(self, ctx: Context, max_batch, max_pixels):
        self.ctx = ctx
        h = C.c_void_p()
        _chk(ctx.lib.mbn_components_create(ctx.h, max_batch, max_pixels, C.byref(h)), ctx.last_error())
        self.h = h
        if not hasattr(ctx, "_resizers"):
            ctx._resizers = []
        ctx._resizers.append(self)

    def close(self):
        if self.h:
            self.ctx.lib.mbn_components_destroy(self.h)
            self.h = None


class RaggedReadout:
    """mbn_ragged_readout_create / _set / mbn_resample_argmax_ragged_f32: the read-out of up to max_batch images of one coarse shape, each to its
    own rows x cols at its own place, in ONE launch. set() takes (dst_offset, rows, cols) tuples (element offsets from the labels / score pointers
    of run()); a refused set raises and leaves the previous one in place."""

    def __init__(self, ctx: Context, max_batch):
        self.ctx = ctx
        self.batch = 0
        h = C.c_void_p()
        _chk(ctx.lib.mbn_ragged_readout_create(ctx.h, max_batch, C.byref(h)), ctx.last_error())
        self.h = h
        if not hasattr(ctx, "_resizers"):
            ctx._resizers = []
        ctx._resizers.append(self)

    def set(self, rows, cols, classes, items, stream=None):
        arr = items if isinstance(items, C.Array) else label_items(items)
        _chk(self.ctx.lib.mbn_ragged_readout_set(self.h, rows, cols, classes, arr, len(arr), stream), self.ctx.last_error())
        self.batch = len(arr)

    def set_window(self, rows, cols, classes, in_rows, in_cols, items, stream=None):
        """mbn_ragged_readout_set_window: (dst_offset, rows, cols, (x, y, iw, ih)) tuples, each image with its own rectangle of the network input."""
        arr = items if isinstance(items, C.Array) else label_window_items(items)
        _chk(self.ctx.lib.mbn_ragged_readout_set_window(self.h, rows, cols, classes, in_rows, in_cols, arr, len(arr), stream), self.ctx.last_error())
        self.batch = len(arr)

    def run(self, labels_ptr, score_ptr, logits_ptr, stream=None):
        _chk(self.ctx.lib.mbn_resample_argmax_ragged_f32(self.h, labels_ptr, score_ptr, logits_ptr, stream), self.ctx.last_error())

    def run_softmax(self, labels_ptr, prob_ptr, score_ptr, logits_ptr, min_prob=0.0, ignore_label=0, stream=None):
        """mbn_resample_softmax_ragged_f32: run() with the probability map (at the items' offsets, like the score) and the threshold; after
        either kind of set."""
        _chk(self.ctx.lib.mbn_resample_softmax_ragged_f32(self.h, labels_ptr, prob_ptr, score_ptr, logits_ptr, min_prob, ignore_label, stream),
             self.ctx.last_error())

    def resample_topk(self, labels_ptr, prob_ptr, score_ptr, logits_ptr, k, plane_stride, min_prob=0.0, ignore_label=0, stream=None):
        """mbn_resample_topk_ragged_f32: the k best classes of every pixel of the set's maps; rank j of item i at j * plane_stride + dst_offset_i
        elements of labels / prob / score. After either kind of set. prob None with min_prob 0: the logit form."""
        _chk(self.ctx.lib.mbn_resample_topk_ragged_f32(self.h, labels_ptr, prob_ptr, score_ptr, logits_ptr, k, plane_stride, min_prob, ignore_label,
                                                       stream), self.ctx.last_error())

    def close(self):
        if self.h:
            self.ctx.lib.mbn_ragged_readout_destroy(self.h)
            self.h = None


class Resizer:
    """mbn_resizer_create_filter / mbn_resize_u8: uint8 HWC images [batch][in_rows][in_cols][3] -> [batch][out_rows][out_cols][3], Pillow's 8-bit
    resize of `box` = (left, upper, right, lower) (None = the whole image) under `filter` (FILTER_*, bilinear by default), byte for byte. One
    geometry and one filter per handle. pad = (R, G, B): the letterbox form (mbn_resizer_create_pad): the whole image with its aspect ratio kept,
    centred on an out_rows x out_cols canvas of that colour (PIL.ImageOps.pad); no box then. view = a View (or (x, y, iw, ih, mirror)) with pad:
    the rectangle given instead of derived, the inner image mirrored when the view says so (mbn_resizer_create_view)."""

    def __init__(self, ctx: Context, in_rows, in_cols, out_rows, out_cols, box=None, filter=FILTER_BILINEAR, pad=None, view=None):
        self.ctx = ctx
        self.filter = filter
        self.shape_in, self.shape_out = (in_rows, in_cols, 3), (out_rows, out_cols, 3)
        h = C.c_void_p()
        if view is not None:
            if box is not None:
                raise ValueError("a view takes the whole image: no box")
            _chk(ctx.lib.mbn_resizer_create_view(ctx.h, filter, in_rows, in_cols, out_rows, out_cols, views([view]),
                                                 _fill3(pad if pad is not None else (0, 0, 0)), C.byref(h)), ctx.last_error())
        elif pad is not None:
            if box is not None:
                raise ValueError("a letterbox takes the whole image: no box")
            _chk(ctx.lib.mbn_resizer_create_pad(ctx.h, filter, in_rows, in_cols, out_rows, out_cols, _fill3(pad), C.byref(h)), ctx.last_error())
        else:
            _chk(ctx.lib.mbn_resizer_create_filter(ctx.h, filter, in_rows, in_cols, _box4(box), out_rows, out_cols, C.byref(h)), ctx.last_error())
        self.h = h
        if not hasattr(ctx, "_resizers"):
            ctx._resizers = []
        ctx._resizers.append(self)

    def run(self, out_ptr, in_ptr, batch, stream=None):
        _chk(self.ctx.lib.mbn_resize_u8(self.h, out_ptr, in_ptr, batch, stream), self.ctx.last_error())

    def close(self):
        if self.h:
            self.ctx.lib.mbn_resizer_destroy(self.h)
            self.h = None


class RaggedResizer:
    """mbn_ragged_resizer_create / _set / mbn_resize_ragged_u8: up to max_batch uint8 HWC images, each with its own rows, cols and box, to one
    [batch][out_rows][out_cols][3] in ONE launch, Pillow's 8-bit resize under `filter` byte for byte (FILTER_NEAREST, _BOX, _BILINEAR, the default,
    or _BICUBIC; hamming and lanczos raise MbnError: EUNSUPPORTED). set() takes (src_offset, rows, cols, box) tuples (byte offsets from the src
    pointer of run(); box None = the whole image). pad = (R, G, B): the letterbox form (mbn_ragged_resizer_create_pad): every image whole, its
    aspect ratio kept, centred on its own out_rows x out_cols canvas of that colour; an item's box must then be None (or the whole image)."""

    def __init__(self, ctx: Context, max_batch, out_rows, out_cols, filter=FILTER_BILINEAR, pad=None):
        self.ctx = ctx
        self.filter = filter
        self.shape_out = (out_rows, out_cols, 3)
        self.batch = 0
        h = C.c_void_p()
        if pad is not None:
            _chk(ctx.lib.mbn_ragged_resizer_create_pad(ctx.h, filter, max_batch, out_rows, out_cols, _fill3(pad), C.byref(h)), ctx.last_error())
        else:
            _chk(ctx.lib.mbn_ragged_resizer_create_filter(ctx.h, filter, max_batch, out_rows, out_cols, C.byref(h)), ctx.last_error())
        self.h = h
        if not hasattr(ctx, "_resizers"):
            ctx._resizers = []
        ctx._resizers.append(self)

    def set(self, items, stream=None):
        self.batch = 0
        arr = items if isinstance(items, C.Array) else resize_items(items)
        _chk(self.ctx.lib.mbn_ragged_resizer_set(self.h, arr, len(arr), stream), self.ctx.last_error())
        self.batch = len(arr)

    def run(self, out_ptr, src_ptr, stream=None):
        _chk(self.ctx.lib.mbn_resize_ragged_u8(self.h, out_ptr, src_ptr, stream), self.ctx.last_error())

    def close(self):
        if self.h:
            self.ctx.lib.mbn_ragged_resizer_destroy(self.h)
            self.h = None


def resize_taps_device(ctx, in_size, b0, b1, out_size, filter=FILTER_BILINEAR):
    """mbn_resize_taps_device_filter: the kernel's own tap function for one axis, downloaded: (first, count, weights [out_size][ksize]) int32."""
    ks = resize_ksize(in_size, b0, b1, out_size, ctx.lib, filter)
    d_f, d_c, d_w = ctx.alloc(4 * out_size), ctx.alloc(4 * out_size), ctx.alloc(4 * out_size * ks)
    rc = ctx.lib.mbn_resize_taps_device_filter(ctx.h, filter, in_size, b0, b1, out_size, d_f.ptr, d_c.ptr, d_w.ptr)
    if rc < 0:
        for b in (d_f, d_c, d_w):
            b.free()
        raise MbnError(rc, "resize_taps_device")
    assert rc == ks
    ctx.sync()
    out = d_f.download((out_size,), np.int32), d_c.download((out_size,), np.int32), d_w.download((out_size, ks), np.int32)
    for b in (d_f, d_c, d_w):
        b.free()
    return out


def input_hw(res):
    """(rows, cols) of a `res` argument: an int is a square side, a pair is (rows, cols)."""
    if isinstance(res, (tuple, list)):
        rows, cols = res
        return int(rows), int(cols)
    return int(res), int(res)


def plan_build(alpha=1.0, res=224, classes=1000, lib=None, output_stride=32) -> Plan:
    """mbn_plan_build; res = (rows, cols) builds a rows x cols plan (mbn_plan_build_hw); output_stride 16 / 8 (or anything but 32)
    goes through mbn_plan_build_os: the late stride-2 depthwise layers stop subsampling, the ones behind them are dilated."""
    p = Plan()
    lib = lib or host_lib()
    if output_stride != 32:
        _chk(lib.mbn_plan_build_os(alpha, *input_hw(res), classes, output_stride, C.byref(p)))
    elif isinstance(res, (tuple, list)):
        _chk(lib.mbn_plan_build_hw(alpha, *input_hw(res), classes, C.byref(p)))
    else:
        _chk(lib.mbn_plan_build(alpha, res, classes, C.byref(p)))
    return p


def quantize_i8(plan, blob, scales=None, lib=None):
    """mbn_quantize_i8: the I8 parameters of `plan` from its fp32 blob with activation scales `scales` (plan.n_layers values, None = the
    defaults 6/255). Returns (I8Params, i8 blob as a uint8 array of params.blob_bytes)."""
    lib = lib or host_lib()
    blob = np.ascontiguousarray(blob, np.float32)
    sc = None if scales is None else np.ascontiguousarray(scales, np.float32)
    if sc is not None and sc.size != plan.n_layers:
        raise ValueError("need %d scales" % plan.n_layers)
    p = I8Params()
    _chk(lib.mbn_quantize_i8(C.byref(plan), None, None if sc is None else sc.ctypes.data, C.byref(p), None))
    out = np.zeros(max(1, p.blob_bytes), np.uint8)
    _chk(lib.mbn_quantize_i8(C.byref(plan), blob.ctypes.data, None if sc is None else sc.ctypes.data, C.byref(p), out.ctypes.data))
    return p, out[:p.blob_bytes]


class HostWeights:
    """mbn_weights_from_h5 result; .blob is a numpy view of the packed fp32 parameters. res = (rows, cols): a rows x cols plan
    (mbn_weights_from_h5_hw), the same blob; output_stride 16 / 8: the plan of mbn_plan_build_os (mbn_weights_from_h5_os), the same blob."""

    def __init__(self, path, alpha=0.0, res=224, lib=None, output_stride=32):
        self.lib = lib or host_lib()
        self.w = Weights()
        if output_stride != 32:
            _chk(self.lib.mbn_weights_from_h5_os(path.encode(), alpha, *input_hw(res), output_stride, C.byref(self.w)), path)
        elif isinstance(res, (tuple, list)):
            _chk(self.lib.mbn_weights_from_h5_hw(path.encode(), alpha, *input_hw(res), C.byref(self.w)), path)
        else:
            _chk(self.lib.mbn_weights_from_h5(path.encode(), alpha, res, C.byref(self.w)), path)
        self.plan = self.w.plan
        self.blob = np.ctypeslib.as_array(self.w.blob, shape=(self.plan.blob_floats,))

    def free(self):
        self.lib.mbn_weights_free(C.byref(self.w))


def synthetic_h5(path, alpha=1.0, classes=1000, seed=0xC0FFEE, lib=None):
    _chk((lib or host_lib()).mbn_weights_synthetic_h5(path.encode(), alpha, classes, seed), path)


class Net:
    """mbn_net_*: the whole-network runner. `blob` may be a numpy array (uploaded once) or a device pointer."""

    def __init__(self, ctx: Context, plan: Plan, blob, max_batch: int):
        self.ctx, self.plan, self.max_batch = ctx, plan, max_batch
        h = C.c_void_p()
        if isinstance(blob, np.ndarray):
            self._dev_blob = ctx.to_device(np.ascontiguousarray(blob, np.float32))
            dev = self._dev_blob.ptr
        else:
            dev = int(blob)
        _chk(ctx.lib.mbn_net_create_from_device_blob(ctx.h, C.byref(plan), dev, max_batch, C.byref(h)), ctx.last_error())
        self.h = h

    def forward(self, images_ptr, out_ptr, batch, last_layer=0):
        _chk(self.ctx.lib.mbn_net_forward(self.h, images_ptr, out_ptr, batch, last_layer), self.ctx.last_error())

    def forward_timed(self, images_ptr, out_ptr, batch):
        ms = (C.c_float * MAX_LAYERS)()
        _chk(self.ctx.lib.mbn_net_forward_timed(self.h, images_ptr, out_ptr, batch, ms, MAX_LAYERS), self.ctx.last_error())
        return [ms[i] for i in range(self.plan.n_layers)]

    def set_streams(self, n, free_running=False):
        _chk(self.ctx.lib.mbn_net_set_streams(self.h, n), self.ctx.last_error())
        _chk(self.ctx.lib.mbn_net_set_free_running(self.h, int(free_running)))

    def set_fuse_stem(self, enabled=True):
        _chk(self.ctx.lib.mbn_net_set_fuse_stem(self.h, int(enabled)))

    def fused_layers(self, last_layer=0) -> int:
        n = C.c_int()
        _chk(self.ctx.lib.mbn_net_fused_layers(self.h, last_layer, C.byref(n)))
        return n.value

    def classify(self, images_dev, batch, k, topk_idx_dev, topk_prob_dev):
        _chk(self.ctx.lib.mbn_net_classify(self.h, images_dev, batch, k, topk_idx_dev, topk_prob_dev), self.ctx.last_error())

    def forward_dense(self, images_ptr, out_ptr, batch):
        """The FC at every pixel of the map in front of the pool: out [batch][h][w][classes] fp32 (mbn_net_forward_dense)."""
        _chk(self.ctx.lib.mbn_net_forward_dense(self.h, images_ptr, out_ptr, batch), self.ctx.last_error())

    def segment(self, images_ptr, batch, labels_ptr, score_ptr=None):
        """forward_dense + bilinear upsample to the input size + argmax: int32 labels (and fp32 scores) [batch][rows][cols] (mbn_net_segment)."""
        _chk(self.ctx.lib.mbn_net_segment(self.h, images_ptr, batch, labels_ptr, score_ptr), self.ctx.last_error())

    def segment_to(self, images_ptr, batch, out_rows, out_cols, labels_ptr, score_ptr=None):
        """forward_dense + bilinear resample to out_rows x out_cols + argmax: int32 labels (and fp32 scores) [batch][out_rows][out_cols]
        (mbn_net_segment_to): the label map at the source resolution of images that went through resize_input(..., FIT_STRETCH)."""
        _chk(self.ctx.lib.mbn_net_segment_to(self.h, images_ptr, batch, out_rows, out_cols, labels_ptr, score_ptr), self.ctx.last_error())

    def segment_images(self, src_ptr, offsets, rows, cols, labels_ptr, dst_offsets, score_ptr=None):
        """mbn_net_segment_images: image i is uint8 [rows[i]][cols[i]][3] at src_ptr + offsets[i]; stretch resize, forward_dense and one ragged
        read-out: its labels (and scores) [rows[i]][cols[i]] at element dst_offsets[i] of labels_ptr (score_ptr). Needs set_input_u8()."""
        n = len(offsets)
        assert len(rows) == n and len(cols) == n and len(dst_offsets) == n
        _chk(self.ctx.lib.mbn_net_segment_images(self.h, src_ptr, (C.c_int64 * n)(*[int(v) for v in offsets]), (C.c_int32 * n)(*[int(v) for v in rows]),
                                                 (C.c_int32 * n)(*[int(v) for v in cols]), n, labels_ptr, (C.c_int64 * n)(*[int(v) for v in dst_offsets]),
                                                 score_ptr), self.ctx.last_error())

    def segment_fit(self, src_ptr, batch, in_rows, in_cols, fit, labels_ptr, score_ptr=None):
        """mbn_net_segment_fit: uint8 sources [batch][in_rows][in_cols][3] -> resize_input(fit), forward_dense and the read-out to the source size:
        labels (and scores) [batch][in_rows][in_cols]. FIT_STRETCH or FIT_PAD (the window read-out of fit_pad's rectangle). Needs set_input_u8()."""
        _chk(self.ctx.lib.mbn_net_segment_fit(self.h, src_ptr, batch, in_rows, in_cols, fit, labels_ptr, score_ptr), self.ctx.last_error())

    def segment_images_fit(self, src_ptr, offsets, rows, cols, fit, labels_ptr, dst_offsets, score_ptr=None):
        """mbn_net_segment_images_fit: segment_images under FIT_STRETCH or FIT_PAD (one ragged window read-out, each image's own rectangle)."""
        n = len(offsets)
        assert len(rows) == n and len(cols) == n and len(dst_offsets) == n
        _chk(self.ctx.lib.mbn_net_segment_images_fit(self.h, src_ptr, (C.c_int64 * n)(*[int(v) for v in offsets]),
                                                     (C.c_int32 * n)(*[int(v) for v in rows]), (C.c_int32 * n)(*[int(v) for v in cols]), n, fit,
                                                     labels_ptr, (C.c_int64 * n)(*[int(v) for v in dst_offsets]), score_ptr), self.ctx.last_error())

    def segment_prob_to(self, images_ptr, batch, out_rows, out_cols, labels_ptr, prob_ptr, min_prob=0.0, ignore_label=0):
        """mbn_net_segment_prob_to: segment_to with the softmax read-out: int32 labels and the fp32 probability of the winning class
        [batch][out_rows][out_cols]; a pixel below min_prob holds ignore_label. prob_ptr may be None only with min_prob > 0."""
        _chk(self.ctx.lib.mbn_net_segment_prob_to(self.h, images_ptr, batch, out_rows, out_cols, labels_ptr, prob_ptr, min_prob, ignore_label),
             self.ctx.last_error())

    def segment_prob_fit(self, src_ptr, batch, in_rows, in_cols, fit, labels_ptr, prob_ptr, min_prob=0.0, ignore_label=0):
        """mbn_net_segment_prob_fit: segment_fit (FIT_STRETCH or FIT_PAD) with the softmax read-out of segment_prob_to."""
        _chk(self.ctx.lib.mbn_net_segment_prob_fit(self.h, src_ptr, batch, in_rows, in_cols, fit, labels_ptr, prob_ptr, min_prob, ignore_label),
             self.ctx.last_error())

    def segment_prob_images_fit(self, src_ptr, offsets, rows, cols, fit, labels_ptr, dst_offsets, prob_ptr, min_prob=0.0, ignore_label=0):
        """mbn_net_segment_prob_images_fit: segment_images_fit with the softmax read-out; image i's probabilities at prob_ptr + dst_offsets[i]."""
        n = len(offsets)
        assert len(rows) == n and len(cols) == n and len(dst_offsets) == n
        _chk(self.ctx.lib.mbn_net_segment_prob_images_fit(self.h, src_ptr, (C.c_int64 * n)(*[int(v) for v in offsets]),
                                                          (C.c_int32 * n)(*[int(v) for v in rows]), (C.c_int32 * n)(*[int(v) for v in cols]), n, fit,
                                                          labels_ptr, (C.c_int64 * n)(*[int(v) for v in dst_offsets]), prob_ptr, min_prob,
                                                          ignore_label), self.ctx.last_error())

    def segment_topk_fit(self, src_ptr, batch, in_rows, in_cols, fit, k, labels_ptr, prob_ptr=None, score_ptr=None, min_prob=0.0, ignore_label=0):
        """mbn_net_segment_topk_fit: segment_prob_fit with the top-k read-out (Context.resample_topk): labels, prob and score are rank-major
        [k][batch][in_rows][in_cols], plane 0 the map of segment_prob_fit. prob None with min_prob 0: the logit form."""
        _chk(self.ctx.lib.mbn_net_segment_topk_fit(self.h, src_ptr, batch, in_rows, in_cols, fit, k, labels_ptr, prob_ptr, score_ptr, min_prob,
                                                   ignore_label), self.ctx.last_error())

    def segment_topk_images_fit(self, src_ptr, offsets, rows, cols, fit, k, plane_stride, labels_ptr, dst_offsets, prob_ptr=None, score_ptr=None,
                                min_prob=0.0, ignore_label=0):
        """mbn_net_segment_topk_images_fit: segment_prob_images_fit with the top-k read-out; rank j of image i at j * plane_stride + dst_offsets[i]
        elements of labels / prob / score."""
        n = len(offsets)
        assert len(rows) == n and len(cols) == n and len(dst_offsets) == n
        _chk(self.ctx.lib.mbn_net_segment_topk_images_fit(self.h, src_ptr, (C.c_int64 * n)(*[int(v) for v in offsets]),
                                                          (C.c_int32 * n)(*[int(v) for v in rows]), (C.c_int32 * n)(*[int(v) for v in cols]), n, fit, k,
                                                          plane_stride, labels_ptr, (C.c_int64 * n)(*[int(v) for v in dst_offsets]), prob_ptr,
                                                          score_ptr, min_prob, ignore_label), self.ctx.last_error())

    def segment_topk_score(self, labels_ptr, truth_ptr, truth_bytes, ranks_ptr):
        """mbn_net_segment_topk_score: ranks (uint64 [classes + 1][k + 1]) += the rank score of the k planes the most recent successful segment call
        wrote (Context.topk_rank); raises EINVAL when that call was not a top-k call."""
        _chk(self.ctx.lib.mbn_net_segment_topk_score(self.h, labels_ptr, truth_ptr, truth_bytes, ranks_ptr), self.ctx.last_error())

    def segment_calibration(self, labels_ptr, prob_ptr, truth_ptr, truth_bytes, bins, calib_ptr):
        """mbn_net_segment_calibration: calib (uint64 [bins + 1][4]) += the calibration table of the maps and probabilities the most recent successful
        segment call wrote (Context.calibration; the net's own set after an image call), with the plan's classes."""
        _chk(self.ctx.lib.mbn_net_segment_calibration(self.h, labels_ptr, prob_ptr, truth_ptr, truth_bytes, bins, calib_ptr), self.ctx.last_error())

    def segment_nll(self, truth_ptr, truth_bytes, inv_temps, table_ptr, nll_ptr=None, brier_ptr=None, plane_stride=0):
        """mbn_net_segment_nll: table (uint64 [temps][classes + 1][4]) += the NLL / Brier table of the probabilities of the most recent successful
        segment call, read out again from the net's dense logits (Context.resample_nll; the net's own set after an image call, which reads
        plane_stride). Raises EUNSUPPORTED after a views or slide call, EINVAL before any call."""
        arr, temps = _inv_temps(inv_temps)
        _chk(self.ctx.lib.mbn_net_segment_nll(self.h, truth_ptr, truth_bytes, arr, temps, table_ptr, nll_ptr, brier_ptr, plane_stride),
             self.ctx.last_error())

    def resize_views(self, src_ptr, batch, in_rows, in_cols, scales, mirrors) -> int:
        """mbn_net_resize_views: uint8 sources [batch][in_rows][in_cols][3] -> the net's staging buffer, view-major: view k = fit_view(scales[k],
        mirrors[k]) of every image at images k * batch .. (its device pointer is returned). batch * views <= max_batch."""
        n = len(scales)
        assert len(mirrors) == n
        p = C.c_void_p()
        _chk(self.ctx.lib.mbn_net_resize_views(self.h, src_ptr, batch, in_rows, in_cols, (C.c_float * n)(*[float(v) for v in scales]),
                                               (C.c_int32 * n)(*[int(v) for v in mirrors]), n, C.byref(p)), self.ctx.last_error())
        return p.value

    def segment_views_fit(self, src_ptr, batch, in_rows, in_cols, scales, mirrors, labels_ptr, prob_ptr=None, score_ptr=None, min_prob=0.0,
                          ignore_label=0):
        """mbn_net_segment_views_fit: test-time augmentation through the letterbox: resize_views, ONE forward_dense of batch * views images and ONE
        ensemble read-out (Context.resample_ensemble) to the source size: labels, prob and score [batch][in_rows][in_cols]. Needs set_input_u8()."""
        n = len(scales)
        assert len(mirrors) == n
        _chk(self.ctx.lib.mbn_net_segment_views_fit(self.h, src_ptr, batch, in_rows, in_cols, (C.c_float * n)(*[float(v) for v in scales]),
                                                    (C.c_int32 * n)(*[int(v) for v in mirrors]), n, labels_ptr, prob_ptr, score_ptr, min_prob,
                                                    ignore_label), self.ctx.last_error())

    def resize_tiles(self, src_ptr, batch, in_rows, in_cols, plan) -> int:
        """mbn_net_resize_tiles: uint8 sources [batch][in_rows][in_cols][3] -> the net's staging buffer, image-major: image b's tile (iy, ix) of
        `plan` at image b * ny * nx + iy * nx + ix (its device pointer is returned). batch * tiles <= max_batch."""
        p = C.c_void_p()
        _chk(self.ctx.lib.mbn_net_resize_tiles(self.h, src_ptr, batch, in_rows, in_cols, C.byref(slide(plan)), C.byref(p)), self.ctx.last_error())
        return p.value

    def segment_slide(self, src_ptr, batch, in_rows, in_cols, tile, stride, labels_ptr, prob_ptr=None, score_ptr=None, min_prob=0.0, ignore_label=0):
        """mbn_net_segment_slide: sliding-window segmentation: tile = (rows, cols) crops at stride = (rows, cols), resize_tiles, ONE forward_dense
        of batch * tiles images and ONE slide read-out (Context.resample_slide) to the source size: labels, prob and score
        [batch][in_rows][in_cols]. Needs set_input_u8()."""
        _chk(self.ctx.lib.mbn_net_segment_slide(self.h, src_ptr, batch, in_rows, in_cols, tile[0], tile[1], stride[0], stride[1], labels_ptr, prob_ptr,
                                                score_ptr, min_prob, ignore_label), self.ctx.last_error())

    def segment_score(self, labels_ptr, truth_ptr, truth_bytes, counts_ptr):
        """mbn_net_segment_score: counts (uint64 [classes + 1][classes + 1]) += the confusion matrix of the maps the most recent successful
        source-size segment call wrote against truth (uint8 or int32, at the labels' element offsets)."""
        _chk(self.ctx.lib.mbn_net_segment_score(self.h, labels_ptr, truth_ptr, truth_bytes, counts_ptr), self.ctx.last_error())

    def segment_boundary_score(self, labels_ptr, truth_ptr, truth_bytes, trimap_ptr, biou_ptr, ratio=0.02, d=0, edge=1):
        """mbn_net_segment_boundary_score: the boundary score of the maps the most recent successful source-size segment call wrote; d > 0 is a
        fixed half-width, d = 0 takes ratio (per image after an image call)."""
        _chk(self.ctx.lib.mbn_net_segment_boundary_score(self.h, labels_ptr, truth_ptr, truth_bytes, trimap_ptr, biou_ptr, ratio, d, edge),
             self.ctx.last_error())

    def segment_boundary_depth(self, labels_ptr, depth_ptr, ratio=0.02, d=0, edge=1):
        """mbn_net_segment_boundary_depth: the band (depth uint8) of those maps, at the labels' element offsets."""
        _chk(self.ctx.lib.mbn_net_segment_boundary_depth(self.h, labels_ptr, depth_ptr, ratio, d, edge), self.ctx.last_error())

    def segment_surface(self, labels_ptr, truth_ptr, truth_bytes, surf_ptr, bins=64, edge=1, dist2_ptr=None):
        """mbn_net_segment_surface: surf (uint64 [classes][2][SURFACE_HEAD + bins]) += the surface-distance table of the maps the most recent
        successful source-size segment call wrote against truth; dist2 (uint32 at the labels' element offsets) or None."""
        _chk(self.ctx.lib.mbn_net_segment_surface(self.h, labels_ptr, truth_ptr, truth_bytes, bins, edge, surf_ptr, dist2_ptr),
             self.ctx.last_error())

    def segment_panoptic(self, labels_ptr, truth_ptr, truth_bytes, pq_ptr, scored_ptr, connectivity=4, min_area=1):
        """mbn_net_segment_panoptic: pq (uint64 [classes][4]) += the panoptic score of the maps the most recent successful source-size segment call
        wrote against truth (components on both, then Context.panoptic); scored (int32 [batch]) says which images were scored."""
        _chk(self.ctx.lib.mbn_net_segment_panoptic(self.h, labels_ptr, truth_ptr, truth_bytes, connectivity, min_area, pq_ptr, scored_ptr),
             self.ctx.last_error())

    def set_panoptic_regions(self, max_regions):
        """mbn_net_set_panoptic_regions: the table size of both sides of segment_panoptic (NET_PANOPTIC_REGIONS until it is called)."""
        _chk(self.ctx.lib.mbn_net_set_panoptic_regions(self.h, max_regions), self.ctx.last_error())

    def segment_regions(self, labels_ptr, n_regions_ptr, comp_ptr=None, regions_ptr=None, labels_out_ptr=None, connectivity=4, min_area=1,
                        ignore_label=0, max_regions=0):
        """mbn_net_segment_regions: the regions of the maps the most recent successful source-size segment call wrote (Context.components, or
        components_ragged on the net's own set after an image call); classes is the plan's."""
        _chk(self.ctx.lib.mbn_net_segment_regions(self.h, labels_ptr, comp_ptr, regions_ptr, n_regions_ptr, labels_out_ptr, connectivity, min_area,
                                                  ignore_label, max_regions), self.ctx.last_error())

    def resize_input(self, src_ptr, batch, in_rows, in_cols, fit=FIT_CROP, crop_fraction=1.0) -> int:
        """mbn_net_resize_input: uint8 images [batch][in_rows][in_cols][3] of any size -> the net's staging buffer [batch][rows][cols][3] (its
        device pointer is returned): the `images` of forward / classify / forward_dense / segment under set_input_u8(). fit: FIT_CROP, FIT_STRETCH
        or FIT_PAD (the letterbox in the net's pad colour; crop_fraction is ignored)."""
        p = C.c_void_p()
        _chk(self.ctx.lib.mbn_net_resize_input(self.h, src_ptr, batch, in_rows, in_cols, fit, crop_fraction, C.byref(p)), self.ctx.last_error())
        return p.value

    def resize_inputs(self, src_ptr, offsets, rows, cols, fit=FIT_CROP, crop_fraction=1.0) -> int:
        """mbn_net_resize_inputs: image i is uint8 [rows[i]][cols[i]][3] at src_ptr + offsets[i]; all of them -> the net's staging buffer in one
        ragged launch (its device pointer is returned), each through its own fit box."""
        n = len(offsets)
        assert len(rows) == n and len(cols) == n
        p = C.c_void_p()
        _chk(self.ctx.lib.mbn_net_resize_inputs(self.h, src_ptr, (C.c_int64 * n)(*[int(v) for v in offsets]), (C.c_int32 * n)(*[int(v) for v in rows]),
                                                (C.c_int32 * n)(*[int(v) for v in cols]), n, fit, crop_fraction, C.byref(p)), self.ctx.last_error())
        return p.value

    def set_resize_filter(self, filter):
        """mbn_net_set_resize_filter: FILTER_* of resize_input / resize_inputs / segment_images (bilinear until it is called)."""
        _chk(self.ctx.lib.mbn_net_set_resize_filter(self.h, int(filter)), "set_resize_filter(%r)" % (filter,))

    def set_pad_color(self, r, g, b):
        """mbn_net_set_pad_color: the border of resize_input / resize_inputs under FIT_PAD (black until it is called)."""
        _chk(self.ctx.lib.mbn_net_set_pad_color(self.h, int(r), int(g), int(b)), "set_pad_color(%r, %r, %r)" % (r, g, b))

    def pad_color(self):
        r, g, b = C.c_int(), C.c_int(), C.c_int()
        _chk(self.ctx.lib.mbn_net_get_pad_color(self.h, C.byref(r), C.byref(g), C.byref(b)))
        return r.value, g.value, b.value

    def resize_filter(self) -> int:
        f = C.c_int()
        _chk(self.ctx.lib.mbn_net_get_resize_filter(self.h, C.byref(f)))
        return f.value

    def set_input_u8(self, enabled=True):
        _chk(self.ctx.lib.mbn_net_set_input_u8(self.h, int(enabled)))

    def set_fuse_blocks(self, mask):
        _chk(self.ctx.lib.mbn_net_set_fuse_blocks(self.h, int(mask)))

    def reset_fuse_blocks(self):
        _chk(self.ctx.lib.mbn_net_reset_fuse_blocks(self.h))

    def set_fuse_tail(self, enabled=True):
        _chk(self.ctx.lib.mbn_net_set_fuse_tail(self.h, int(enabled)))

    def set_fuse_resident(self, enabled=True):
        """Runs of equal small-map bf16 blocks as one launch with the map resident in LDS (default on)."""
        _chk(self.ctx.lib.mbn_net_set_fuse_resident(self.h, int(enabled)))

    def get_fuse_blocks(self) -> int:
        m = C.c_uint()
        _chk(self.ctx.lib.mbn_net_get_fuse_blocks(self.h, C.byref(m)))
        return m.value

    def launches(self, batch, last_layer=0):
        """[(first_layer, n_layers), ...] of the launches one forward issues per (sub-)batch."""
        cap = 64
        a, b, n = (C.c_int * cap)(), (C.c_int * cap)(), C.c_int()
        _chk(self.ctx.lib.mbn_net_launches(self.h, batch, last_layer, a, b, cap, C.byref(n)))
        return [(a[i], b[i]) for i in range(min(n.value, cap))]

    def set_graph(self, enabled=True):
        _chk(self.ctx.lib.mbn_net_set_graph(self.h, int(enabled)), self.ctx.last_error())

    def set_dtype(self, dtype):
        _chk(self.ctx.lib.mbn_net_set_dtype(self.h, dtype), self.ctx.last_error())
        self.dtype = dtype                # only once the net has switched (I8 can refuse a plan)

    def set_act_scales_i8(self, scales):
        """I8 activation scales s_l, one per layer (pool / FC entries ignored); re-quantizes in I8 mode."""
        a = (C.c_float * self.plan.n_layers)(*[float(x) for x in scales])
        _chk(self.ctx.lib.mbn_net_set_act_scales_i8(self.h, a, self.plan.n_layers), self.ctx.last_error())

    def get_act_scales_i8(self) -> np.ndarray:
        a = (C.c_float * self.plan.n_layers)()
        _chk(self.ctx.lib.mbn_net_get_act_scales_i8(self.h, a, self.plan.n_layers))
        return np.array(a[:], np.float32)

    def calibrate_i8(self, images_ptr, batch):
        """s_l = min(6, max_l) / 255 from an fp32 forward of `batch` device images; the dtype and other settings stay."""
        _chk(self.ctx.lib.mbn_net_calibrate_i8(self.h, images_ptr, batch), self.ctx.last_error())

    def keep_activations(self, keep=True):
        _chk(self.ctx.lib.mbn_net_set_keep_activations(self.h, int(keep)))

    def layer_output(self, index, batch, images=None) -> np.ndarray:
        """Kept activation of layer `index` (1-based): the whole batch, or only the listed images (full-size batches: a few images
        of an 800 MB tensor)."""
        p, n = C.c_void_p(), C.c_size_t()
        _chk(self.ctx.lib.mbn_net_layer_output(self.h, index, C.byref(p), C.byref(n)))
        l = self.plan.layer[index - 1]
        dt = getattr(self, "dtype", DT_F32)
        bf = dt == DT_BF16 and l.kind != L_FC
        per = (l.out_rows, l.out_cols, l.out_ch)
        et = np.uint16 if bf else np.uint8 if (dt == DT_I8 and l.kind != L_FC) else np.float32
        raw = np.empty((batch if images is None else len(images),) + per, et)
        if images is None:
            _chk(self.ctx.lib.mbn_download(self.ctx.h, raw.ctypes.data, p, raw.nbytes))
        else:
            step = raw[0].nbytes
            for j, im in enumerate(images):
                assert 0 <= im < batch
                _chk(self.ctx.lib.mbn_download(self.ctx.h, raw[j].ctypes.data, p.value + im * step, step))
        return bf16_bits_to_f32(raw) if bf else raw

    def destroy(self):
        if self.h:
            self.ctx.lib.mbn_net_destroy(self.h)
            self.h = None
