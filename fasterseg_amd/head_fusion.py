"""Which 1x1 convolutions of a traced eval-mode network can run inside the launch of the 3x3 / stride-1 convolution in front of them
(csrc/conv3x3_pw.hip, fs_conv3x3_pw_fwd).  Host only: the pass looks at op kinds, shapes and producer / consumer edges.

The tail of every derived network is ffm.conv_1x1 (BN, ReLU) -> heads.conv_3x3 (BN, ReLU) -> heads.conv_1x1 (+bias) (model_seg.py:345,
seg_oprs.py:22,245) and an arm of `_arm_up_refine` (model_seg.py:322-334) is a 3x3 whose only eval-mode reader is a 1x1.  One pattern
is fused:

    3x3 -> 1x1

The rule: the 3x3's map has exactly ONE consumer and is not the engine's output - in train mode the heads' 3x3 feeds a second head, and
then nothing is fused.  Channel limits are the kernel's (the block owns every channel of its pixel tile).  `1x1(BN, ReLU) -> 3x3` (the
ffm 1x1 in front of the head's 3x3) is NOT matched: the launch form that recomputes the 1x1 on the 3x3's halo was built and measured no
faster than the two launches, so the 1x1 in front stays a launch of its own."""

MAX_CHANNELS = 128


def _live(op):
    return not op.get("dead")


def _is_c3(op):
    return (op["kind"] == "conv" and _live(op) and op["k"] == 3 and op["stride"] == 1 and op["pad"] == 1 and op.get("vres") is None
            and op.get("fold") is None and op["cout"] <= MAX_CHANNELS and op["cout"] % 8 == 0)


def _is_pw(op):
    return (op["kind"] == "conv" and _live(op) and op["k"] == 1 and op["stride"] == 1 and op["pad"] == 0 and op.get("vres") is None
            and op["cout"] <= MAX_CHANNELS)


def consumers_of(ops):
    cons = {}
    for idx, op in enumerate(ops):
        if not _live(op):
            continue
        for s_ in (op["inputs"] if op["kind"] == "cat" else [op["x"]]):
            cons.setdefault(s_.id, []).append(idx)
    return cons


def match(ops, out_sym):
    """[dict(conv=op index of the 3x3, post=op index of the 1x1)], in op order."""
    cons = consumers_of(ops)
    found = []
    for ic, C in enumerate(ops):
        if not _is_c3(C) or C["out"] is out_sym:
            continue
        readers = cons.get(C["out"].id, [])
        if len(readers) != 1:
            continue
        Q = ops[readers[0]]
        if _is_pw(Q) and Q["x"] is C["out"] and Q["cin"] == C["cout"]:
            found.append(dict(conv=ic, post=readers[0]))
    return found
