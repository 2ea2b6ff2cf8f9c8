"""C ABI of the training losses (tdrn_hip.h section ii-b), no GPU needed: the symbols exist, the workspace queries reject
what the entries reject, and null pointers, bad sizes, misaligned vectors and short workspaces return their codes before
any launch."""
from tdrn_amd import _lib

E_ARG, E_WORKSPACE, E_UNSUPPORTED = -1, -3, -4
p = 4096            # fake non-NULL device pointers (16-byte aligned): these paths return before anything is enqueued


def test_symbols_exist():
    lib = _lib.lib()
    for name in ("tdrn_encode", "tdrn_match_workspace_bytes", "tdrn_match", "tdrn_multibox_loss_workspace_bytes",
                 "tdrn_multibox_loss_forward", "tdrn_multibox_loss_backward"):
        assert hasattr(lib, name)


def test_match_workspace_query_and_entry_agree():
    lib = _lib.lib()
    q = lib.tdrn_match_workspace_bytes
    assert q(4, 6375, 60) > 0 and q(32, 16320, 512) > 0 and q(1, 10, 0) > 0
    for bad in ((0, 6375, 60), (4, 0, 60), (4, 6375, -1), (4, 6375, 513)):
        assert q(*bad) == 0, bad
    nb = q(2, 100, 8)

    def m(truths=p, off=p, T=10, Tmax=8, B=2, pri=p, P=100, arm=None, loc_t=p, conf_t=p, ws=p, wsb=nb):
        return lib.tdrn_match(truths, off, T, Tmax, B, pri, P, arm, 0.5, 0.1, 0.2, loc_t, conf_t, ws, wsb, None)
    assert m(Tmax=513, wsb=1 << 30) == E_UNSUPPORTED
    assert m(wsb=nb - 1) == E_WORKSPACE
    assert m(off=None) == E_ARG
    assert m(pri=None) == E_ARG
    assert m(loc_t=None) == E_ARG
    assert m(conf_t=None) == E_ARG
    assert m(truths=None) == E_ARG                       # NULL truths only with T_total = 0
    assert m(B=0) == E_ARG and m(P=0) == E_ARG and m(T=-1) == E_ARG
    assert m(pri=p + 4) == E_ARG and m(arm=p + 8) == E_ARG and m(loc_t=p + 4) == E_ARG     # 16-byte vectors
    assert m(ws=None) == E_ARG


def test_loss_workspace_query_and_entries_agree():
    lib = _lib.lib()
    q = lib.tdrn_multibox_loss_workspace_bytes
    assert q(32, 6375, 21) > 0 and q(2, 65536, 81) > 0 and q(4, 6375, 0) > 0 and q(1, 10, 1024) > 0
    assert q(4, 6375, 0) < q(4, 6375, 21)
    for bad in ((0, 6375, 21), (4, 0, 21), (4, 6375, -1), (4, 6375, 1025)):
        assert q(*bad) == 0, bad
    nb = q(2, 100, 21)

    def f(loc=p, conf=p, loc_t=p, conf_t=p, B=2, P=100, C=21, negpos=3, loss=p, sel=p, npos=p, ws=p, wsb=nb):
        return lib.tdrn_multibox_loss_forward(loc, conf, loc_t, conf_t, B, P, C, negpos, loss, sel, npos, ws, wsb, None)
    assert f(C=1025, wsb=1 << 30) == E_UNSUPPORTED
    assert f(wsb=nb - 1) == E_WORKSPACE
    assert f(conf=None, wsb=q(2, 100, 0) - 1) == E_WORKSPACE
    for k in ("loc", "loc_t", "conf_t", "loss", "sel", "npos"):
        assert f(**{k: None}) == E_ARG, k
    assert f(C=0) == E_ARG and f(B=0) == E_ARG and f(P=0) == E_ARG and f(negpos=-1) == E_ARG
    assert f(loc=p + 4) == E_ARG and f(loc_t=p + 8) == E_ARG
    assert f(ws=None) == E_ARG

    def b(loc=p, conf=p, loc_t=p, conf_t=p, sel=p, npos=p, g=p, B=2, P=100, C=21, gl=p, gc=p):
        return lib.tdrn_multibox_loss_backward(loc, conf, loc_t, conf_t, sel, npos, g, B, P, C, gl, gc, None)
    for k in ("loc", "loc_t", "conf_t", "sel", "npos", "g", "gl", "gc"):
        assert b(**{k: None}) == E_ARG, k
    assert b(C=1025) == E_UNSUPPORTED
    assert b(C=0) == E_ARG and b(B=0) == E_ARG and b(P=0) == E_ARG
    assert b(gl=p + 4) == E_ARG and b(loc=p + 4) == E_ARG


def test_encode_rejects_misaligned_and_null():
    lib = _lib.lib()
    assert lib.tdrn_encode(None, p, 10, 0.1, 0.2, p, None) == E_ARG
    assert lib.tdrn_encode(p + 4, p, 10, 0.1, 0.2, p, None) == E_ARG
    assert lib.tdrn_encode(p, p, -1, 0.1, 0.2, p, None) == E_ARG
    assert lib.tdrn_encode(p, p, 0, 0.1, 0.2, p, None) == 0
