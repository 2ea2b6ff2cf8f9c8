"""tests/_train_stage_ref.py's method on the training steps of refinedet_vgg and the two SSD4Scale models (test helper; product code
never imports it): tests/_train_stage_dw.py's recorder with conv5x5 as one more kind, and the check of a 5x5 stage under the
dense-conv rule.  Neither of the two older helpers is edited; the kinds they know are delegated to them.

Recorder.  The seven wrappers of _train_stage_dw.Recorder, plus one around tdrn_amd.model.networks.conv5x5 (forward_train looks it up
at call time like the others).  finish() states the recorder's four facts with the module's nn.Conv2d holders counted as 5x5
(kernel_size (5, 5), groups 1), depthwise or dense; each count must equal the number of stages of its kind, and a 5x5 stage's weight
must be a (Cout, Cin, 5, 5) parameter of a holder with padding 2.

The SSD4Scale nets are recorded with TrainWalk._paired_heads = False: the paired form hands conv_offset2d the concatenation of two
parameters, which is no parameter of the module, so "every parameter in exactly one stage" can be stated only for the separate form.
test_gpu_train_trn.py::test_paired_and_separate_heads_agree ties the two forms together.

5x5 stage.  Reference: F.conv2d(padding=2) with autograd on the CPU in float64 from the stage's own recorded input, weight, bias and
grad_output, through _train_stage_ref._check_conv: fp32 |got - ref| <= 1e-4 max|ref|, 16-bit C_ACC S, as for conv2d.
"""
import copy

import _train_stage_dw as W
import _train_stage_ref as R

CONV5X5 = "conv5x5"
KINDS = W.KINDS + (CONV5X5,)
calibrate = W.calibrate
_older_holder_kind = W._holder_kind


def holder_kind(m):
    if type(m).__name__ == "Conv2d" and m.groups == 1 and tuple(m.kernel_size) == (5, 5):
        return CONV5X5
    return _older_holder_kind(m)


def holder_counts(module):
    """{kind: how many holders of the module an op of that kind serves}: what the stage counts must be"""
    counts = {}
    for m in module.modules():
        k = holder_kind(m)
        if k is not None:
            counts[k] = counts.get(k, 0) + 1
    return counts


class Recorder(W.Recorder):
    def __enter__(self):
        super(Recorder, self).__enter__()
        self._saved[CONV5X5] = getattr(self.networks, CONV5X5)
        setattr(self.networks, CONV5X5, self._wrapper(CONV5X5, self._saved[CONV5X5]))
        return self

    def finish(self):
        """_train_stage_dw.Recorder.finish with the 5x5 holders counted as their own kind (its holder rule is a module-level
        function, looked up at call time: replaced for the duration of the call)"""
        saved, W._holder_kind = W._holder_kind, holder_kind
        try:
            stages = super(Recorder, self).finish()
        finally:
            W._holder_kind = saved
        holders = dict(self.module.named_modules())
        for st in stages:
            if st.kind == CONV5X5:
                m = holders[st.name]
                assert holder_kind(m) == CONV5X5 and tuple(m.padding) == (2, 2) and tuple(st.inputs["weight"].shape[2:]) == (5, 5), st
            elif st.kind == "conv2d":
                assert holder_kind(holders[st.name]) == "conv2d", st
        return stages


def _check_conv5x5(st, cancelling, shares):
    twin = copy.copy(st)
    twin.kind, twin.args = "conv2d", dict(st.args, stride=1, padding=2, dilation=1)
    twin.name = "%s (5x5)" % st.name
    R._check_conv(twin, cancelling, shares)


def check_stage(st, cancelling=()):
    """-> [(tensor, worst share of its bound)]; the seven older kinds go to _train_stage_dw.check_stage"""
    if st.kind != CONV5X5:
        return W.check_stage(st, cancelling)
    shares = []
    _check_conv5x5(st, cancelling, shares)
    return shares


def check_stages(stages, cancelling=(), select=None, failures=None):
    """_train_stage_ref.check_stages over the eight kinds -> {kind: (worst share, stage name, tensor)}"""
    worst = {}
    chosen = R.select_stages(stages, select)
    assert chosen, "the selection holds no stage"
    for st in chosen:
        try:
            shares = check_stage(st, cancelling)
        except AssertionError as e:
            if failures is None:
                raise
            failures[st.name] = str(e)
            continue
        for name, share in shares:
            if st.kind not in worst or share > worst[st.kind][0]:
                worst[st.kind] = (share, st.name, name)
    for kind, (share, name, tensor) in sorted(worst.items()):
        print("worst share of a bound, %-16s %.4f (%s %s)" % (kind, share, name, tensor))
    return worst
