"""Print the layer plan of a list of net configurations: parameters, tensors, every op_info field, blob / workspace sizes and the
library's own `plan:` lines (lane, split-K, the kernel at batch 1 / at batch 32, chain index).  CPU only: no GPU, no torch device.  Two builds of the
library plan alike exactly when their outputs are byte-identical:

    TDRN_LIB_PATH=/path/to/other/libtdrn_hip.so python scripts/plan_dump.py | sha256sum
    python scripts/plan_dump.py | sha256sum
"""
import ctypes as C
import itertools
import os
import sys

os.environ["TDRN_PLAN_DUMP"] = "1"
os.dup2(1, 2)                                        # the library prints its `plan:` lines to stderr: one stream, in order
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from tdrn_amd import _lib  # noqa: E402

FIELDS = ("model", "size", "num_classes", "def_groups", "bn", "multihead", "deform", "test_phase", "dtype", "use_refine", "plan_flags")


def configs():
    """Every axis the tests and bench.py construct nets along; v = 1: eight deformable groups (DRN) / deformable heads (ssd4scale)."""
    out = []
    for m, dt, size, mh, bn, v in itertools.product(range(5), range(3), (192, 320, 384, 448, 512), (0, 1), (0, 1), (0, 1)):
        out.append((m, size, 21, 8 if v else 1, bn, mh, v, 1, dt, 0, 0))
    for m, dt, size, mh, v, nc, ref, test in itertools.product(range(5), range(3), (320, 512), (0, 1), (0, 1), (21, 31, 81), (0, 1), (0, 1)):
        out.append((m, size, nc, 8 if v else 1, 1, mh, v, test, dt, ref, 0))
    for m, size, v, bit in itertools.product((_lib.DRN_VGGBN, _lib.DRN_MOBILENET, _lib.SSD4SCALE_MOBILE, _lib.SSD4SCALE_VGG), (320, 512), (0, 1), range(18)):
        out.append((m, size, 21, 1, 1, 0, v, 1, _lib.BF16, 0, 1 << bit))
    return sorted(set(out))


def dump(lib, cfg):
    print("net " + " ".join("%s=%d" % kv for kv in zip(FIELDS, cfg)))
    sys.stdout.flush()
    net = C.c_void_p()
    rc = lib.tdrn_net_create(C.byref(_lib.NetConfig(c7_channel=1024, **dict(zip(FIELDS, cfg)))), C.byref(net))
    if rc != 0:
        print("  create: %d" % rc)
        return
    name, shape, ndim = C.c_char_p(), (C.c_int64 * 4)(), C.c_int()
    for i in range(lib.tdrn_net_param_count(net)):
        lib.tdrn_net_param_info(net, i, C.byref(name), C.byref(shape), C.byref(ndim))
        print("  param %s %s" % (name.value.decode(), list(shape)[:ndim.value]))
    c, h, w = C.c_int(), C.c_int(), C.c_int()
    for i in range(lib.tdrn_net_tensor_count(net)):
        lib.tdrn_net_tensor_info(net, i, C.byref(name), C.byref(c), C.byref(h), C.byref(w))
        print("  tensor %d %r %d %d %d" % (i, name.value.decode(), c.value, h.value, w.value))
    op = _lib.OpInfo()
    for i in range(lib.tdrn_net_op_count(net)):
        lib.tdrn_net_op_info(net, i, C.byref(op))
        vals = [getattr(op, f) for f, _ in _lib.OpInfo._fields_]
        print("  op %d %s" % (i, " ".join(str(list(v)) if hasattr(v, "__len__") and not isinstance(v, bytes) else str(v) for v in vals)))
    print("  weights %d workspace %d %d priors %d" % (lib.tdrn_net_weight_bytes(net), lib.tdrn_net_workspace_bytes(net, 1),
                                                       lib.tdrn_net_workspace_bytes(net, 32), lib.tdrn_net_num_priors(net)))
    sys.stdout.flush()
    lib.tdrn_net_destroy(net)


if __name__ == "__main__":
    todo = configs()
    for cfg in todo:
        dump(_lib.lib(), cfg)
    print("configs %d" % len(todo))
