"""ctypes declarations of the actor unit statistics' entry points (include/parc_netstats.h)."""
import ctypes

c_vp, c_int, c_f, c_i32, c_i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_int32, ctypes.c_int64

MAX_LAYERS = 8      # PARC_NETSTATS_MAX_LAYERS
ROWS = 64           # PARC_NETSTATS_ROWS: rows per workgroup of the partial kernel
COLS = 256          # PARC_NETSTATS_COLS


class NetstatsLayerS(ctypes.Structure):
    """parc_netstats_layer_t"""
    _fields_ = [("act", c_vp), ("dim", c_i32), ("out_abs_sum", c_vp), ("activations", c_vp), ("utility", c_vp)]


class NetstatsTableS(ctypes.Structure):
    """parc_netstats_table_t"""
    _fields_ = [("num_layers", c_i32), ("layer", NetstatsLayerS * MAX_LAYERS)]


def table(layers):
    """layers: (act, dim, out_abs_sum, activations, utility) per layer, the pointers as integers (0 / None = NULL)"""
    t = NetstatsTableS()
    t.num_layers = len(layers)
    for i, (act, dim, s, a, u) in enumerate(layers[:MAX_LAYERS]):
        t.layer[i] = NetstatsLayerS(act or None, int(dim), s or None, a or None, u or None)
    return t


def declare(L):
    L.parc_netstats_abi.restype = c_int
    L.parc_netstats_workspace_floats.restype = c_i64
    L.parc_netstats_workspace_floats.argtypes = [c_i64, NetstatsTableS]
    L.parc_netstats_update.restype = c_int
    L.parc_netstats_update.argtypes = [c_vp, c_i64, NetstatsTableS, c_int, c_vp, c_vp, c_f, c_f, c_vp]
    L.parc_netstats_abs_colsum.restype = c_int
    L.parc_netstats_abs_colsum.argtypes = [c_vp, c_int, c_int, c_vp, c_vp]
    L.parc_netstats_dormant_count.restype = c_int
    L.parc_netstats_dormant_count.argtypes = [c_vp, NetstatsTableS, c_i64, c_vp, c_f, c_vp]
