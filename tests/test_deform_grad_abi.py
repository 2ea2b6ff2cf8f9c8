"""C ABI of the deformable-conv backward (tdrn_hip.h section i-b), no GPU needed: the workspace query mirrors the
forward's shape_check (deform_conv_cuda.c:7-96) and the entries reject what it rejects."""
from tdrn_amd import _lib


def test_deform_backward_workspace_query_mirrors_shape_check():
    lib = _lib.lib()
    q = lambda *a: lib.tdrn_deform_conv_backward_workspace_bytes(*a)
    fwd = lambda *a: lib.tdrn_deform_conv_workspace_bytes(*a, 0)
    cases = [
        ((1, 6, 8, 8, 4, 3, 3, 1, 1, 1, 1, 1, 1, 1), True),
        ((1, 6, 8, 8, 4, 3, 3, 1, 1, 1, 1, 1, 1, 4), False),     # Cin % G != 0
        ((1, 6, 2, 2, 4, 3, 3, 1, 1, 0, 0, 1, 1, 1), False),     # input smaller than kernel
        ((1, 6, 8, 8, 4, 0, 3, 1, 1, 1, 1, 1, 1, 1), False),     # kernel size must be > 0
        ((1, 6, 8, 8, 4, 3, 3, 0, 1, 1, 1, 1, 1, 1), False),     # stride must be > 0
        ((1, 6, 8, 8, 4, 3, 3, 1, 1, 1, 1, 0, 1, 1), False),     # dilation must be > 0
        ((1, 6, 8, 8, 4, 3, 3, 1, 1, -1, 1, 1, 1, 1), False),    # negative padding
        ((0, 6, 8, 8, 4, 3, 3, 1, 1, 1, 1, 1, 1, 1), False),     # empty batch
        ((8, 256, 40, 40, 63, 3, 3, 1, 1, 1, 1, 1, 1, 1), True),  # ODM conf head, 40x40 level
        ((2, 512, 20, 20, 12, 3, 3, 1, 1, 1, 1, 1, 1, 8), True),  # TRN head, 8 deformable groups
    ]
    for args, ok in cases:
        assert (q(*args) > 0) == ok, args
        assert (fwd(*args) > 0) == ok, args


def test_deform_backward_entries_reject_bad_shapes_and_workspace():
    lib = _lib.lib()
    # pointers are only checked for NULL before any launch: fake non-NULL ones never reach a kernel on these paths
    p = 256
    bad = (1, 6, 8, 8, 4, 3, 3, 1, 1, 1, 1, 1, 1, 4)             # N Cin H W Cout kW kH dW dH padW padH dilH dilW G; Cin % G
    assert lib.tdrn_deform_conv_backward_input(p, p, p, p, p, p, *bad, p, 1 << 20, None) == -2
    assert lib.tdrn_deform_conv_backward_parameters(p, p, p, p, *bad, 1.0, p, 1 << 20, None) == -2
    good = (1, 6, 8, 8, 4, 3, 3, 1, 1, 1, 1, 1, 1, 1)
    nb = lib.tdrn_deform_conv_backward_workspace_bytes(*good)
    assert lib.tdrn_deform_conv_backward_input(p, p, p, p, p, p, *good, p, nb - 1, None) == -3
    assert lib.tdrn_deform_conv_backward_parameters(p, p, p, p, *good, 1.0, p, nb - 1, None) == -3
    assert lib.tdrn_deform_conv_backward_input(None, p, p, p, p, p, *good, p, nb, None) == -1
    assert lib.tdrn_deform_conv_backward_parameters(p, p, None, p, *good, 1.0, p, nb, None) == -1
