"""The ResUNet and vocoder plans as chains of their own launches (tests/test_gpu_plan_chains.py, tests/test_plan_chains_host.py).

A whole call -- Engine.resunet_mel, resunet_spec, vocoder -- runs one cached plan; the launch tests run every launch of it as a plan of
its own.  The functions here run those one-launch plans one behind the other, each output handed to the next launch the way the network
is wired, so that a test can hold the whole call to the chain bit for bit: the kernels are deterministic and both sides build their
launches with the same builder functions, so whatever differs is the plan's wiring -- which buffer feeds which launch, in which form,
with which slope, with which split-K rule, and whether two live buffers share bytes of the arena.

Nothing here is read off the plan builders.  The ResUNet's piece order is the network's: oracle/resunet.py (_trunk, encoder_block,
decoder_block, unet_mel, unet_spec_mag), which restates the reference's unet.py / unet_v2.py and modules.py.  The vocoder's wiring follows
the generator of oracle/vocoder.py and the rule of DESIGN.md section 2 for the forms of a tensor, stated from the consumer's side; the
kernel family of a stack and its trunk format are the product's choice and are ASKED of it (Engine.plan_voc_stack, the `info` of the
fused launches), the few lines that restate a rule of vocoder.cpp are marked COPIED.
"""
import torch

from voicefixer_main_amd.engine import MODEL_UNET_MEL, MODEL_UNET_SPEC

ACT_NONE, ACT_LEAKY, ACT_ELU = 0, 1, 2

# ---------------------------------------------------------------------------------------------------------------------------------
# ResUNets
# ---------------------------------------------------------------------------------------------------------------------------------
LEVEL_CHANNELS = (32, 64, 128, 256, 384, 384)   # encoder_block1..6 (unet.py / unet_v2.py: UNetResComplex_100Mb)
UNET_WIDTH = {MODEL_UNET_MEL: 127, MODEL_UNET_SPEC: 1024}   # the trunk's width: the input without its last bin (unet.py:78, unet_v2.py:100)


def short_clip_of(Tpad):
    """The documented split-K rule of a whole ResUNet call (include/vfx_test.h: vfx_op_unet_piece, PlanBuilder::short_clip)."""
    if Tpad <= 128:
        return 1
    if Tpad >= 2048:
        return -(Tpad // 1024)
    return 0


def unet_steps(model):
    """The pieces of the network in the order it evaluates them -> [(piece, arg)].  arg: the channel count for "pool", 1 for the
    spectrogram model's pruned (even-width) upsamplers and its two-output epilogue, else 0."""
    spec = int(model == MODEL_UNET_SPEC)
    steps = [("prep_spec" if spec else "prep_logmel", 0), ("entry", 0)]           # _pad_time, x[..., :-1]; encoder_block1.conv_block1
    for l in range(1, 7):                                                         # encoder_block: four blocks, then the pool
        steps += [("enc%d.%d" % (l, j), 0) for j in range(2 if l == 1 else 1, 5)]
        steps.append(("pool", LEVEL_CHANNELS[l - 1]))
    steps.append(("bott", 0))                                                     # conv_block7
    for d in range(1, 7):                                                         # decoder_block: upsample, cat with the skip, four blocks
        steps.append(("dec%d.up" % d, spec))
        steps += [("dec%d.%d" % (d, j), 0) for j in range(1, 5)]
    steps += [("after", 0), ("final", spec)]                                      # after_conv_block1; after_conv2 and the model's epilogue
    return steps


def unet_geometry(model, T, steps=None):
    """-> [(piece, arg, H, W)]: the (H, W) each piece of unet_steps is given (vfx_plan_unet_piece's arguments) for clips of T frames."""
    Tpad = (T + 63) // 64 * 64
    W0 = UNET_WIDTH[model]
    H, W = Tpad, W0
    out = []
    for piece, arg in (unet_steps(model) if steps is None else steps):
        if piece.startswith("prep") or piece == "final":
            out.append((piece, arg, T, W0))
            continue
        out.append((piece, arg, H, W))
        if piece == "pool":
            H, W = H // 2, W // 2
        elif piece.endswith(".up"):
            H, W = 2 * H, (2 * W if arg else 2 * W + 1)
    return out


def unet_chain(eng, model, x, aux, short_clip=None, swap_dec1=False, check_launches=True):
    """The network of `model` on `eng`, one piece at a time through Engine.op_unet_piece.  x: the linear mel (B, T, 128) or the
    magnitude spectrogram (B, T, 1025); aux: what the epilogue reads beside the trunk -- [mel] or [cos, sin].  -> the outputs of
    "final".  short_clip: every piece's split-K rule (default: the documented rule at this Tpad).  swap_dec1: hand dec1.1 its two
    sources the wrong way round (a negative control).  check_launches: every piece launched what vfx_plan_unet_piece says."""
    B, T = x.shape[:2]
    sc = short_clip_of((T + 63) // 64 * 64) if short_clip is None else short_clip
    skips = []
    y = x
    for piece, arg, H, W in unet_geometry(model, T):
        if piece == "pool":
            skips.append(y)
        if piece.startswith("dec") and piece.endswith(".1"):
            ins = [y, skips.pop()]                      # cat((upsampled, skip)): the skip of level 7 - d
            if swap_dec1 and piece == "dec1.1":
                ins = ins[::-1]
        elif piece == "final":
            ins = [y] + list(aux)
        else:
            ins = [y]
        outs, _, launches = eng.op_unet_piece(piece, ins, arg=arg, short_clip=sc, model=model)
        if check_launches:
            assert launches == eng.plan_unet_piece(piece, B, H, W, arg=arg, short_clip=sc, precision=eng.cfg.precision,
                                                   tuning=eng.cfg.tuning), (piece, H, W, launches)
        y = outs[0] if piece != "final" else outs
    assert not skips
    return y


SMALL, BLOCKS, CONVS = 0, 1, 2


def launch_category(launch):
    """describe_unet_launches reports a plan's small kernels, then its fused blocks, then its convolutions."""
    return {"small": SMALL, "k_conv": CONVS, "k_conv_phased": CONVS}.get(launch["family"], BLOCKS)


def unet_chain_launches(plan_piece, model, B, T, steps=None, short_clip=None):
    """plan_piece = Engine.plan_unet_piece with precision and tuning bound -> the launches of the chain per category, each in chain order."""
    sc = short_clip_of((T + 63) // 64 * 64) if short_clip is None else short_clip
    cats = ([], [], [])
    for piece, arg, H, W in unet_geometry(model, T, steps):
        for launch in plan_piece(piece, B, H, W, arg=arg, short_clip=sc):
            cats[launch_category(launch)].append(launch)
    return cats


# ---------------------------------------------------------------------------------------------------------------------------------
# vocoder
# ---------------------------------------------------------------------------------------------------------------------------------
def _layer(sd, idx, i):
    p = "generator.%d.res_layers.%d." % (idx, i)
    return sd[p + "1.weight"], sd[p + "1.bias"], sd[p + "3.weight"], sd[p + "3.bias"]


def vocoder_chain(eng, sd, mel, cfg=None, last_layer_slope=None, tail_activated=False, log=None):
    """The vocoder of `eng` on the linear mel (B, T, 128), launch by launch through the op_voc_* entry points with the tensors of the
    state dict `sd` -> wav (B, (T + T % 2 + 4) * prod(scales)).  cfg: the layer table (default eng.cfg).

    A tensor between two launches is a dict: raw -- fp32 values (of an fp16 trunk: widened, which loses nothing) or None; f16 -- that
    raw tensor is stored as fp16; act -- the activated form as its producer stored it (Engine.stored_tensor) or None.  The rule, from
    the consumer's side: a convolution reads the ACTIVATED form of its input if the producer wrote one, and then
    the producer applied the CONSUMER's activation -- ELU in the condnet and in front of the k7 convolution, LeakyReLU(res_slope) inside
    a stack, LeakyReLU(up_slope) in front of an upsampler; the raw form is written where a residual add or the tail reads it; the
    fused stack kernels read the raw trunk (fp16 where the plan keeps it so) and apply their activations themselves.

    Negative controls: last_layer_slope -- the slope the last layer in front of an upsampler activates its output with (the rule:
    up_slope); tail_activated -- hand the tail LeakyReLU(x, up_slope) instead of x.  log: a list that receives one line per launch."""
    c = eng.cfg if cfg is None else cfg
    p = eng.precision
    B, T, _ = mel.shape
    Tp = T + T % 2 + 4
    up_slope, res_slope = float(c.voc_up_slope), float(c.voc_res_slope)
    n_stages, base = int(c.voc_n_stages), int(c.voc_dilation_base)
    say = (lambda *a: log.append(a)) if log is not None else (lambda *a: None)

    def stored16(ya):   # the fp32 values an op widened from an fp16 tensor, back as that tensor (exact both ways)
        return ya.to(torch.float16).contiguous()

    x = eng.op_voc_prep(mel, Tp)
    # condnet: Conv1d k3, ELU behind each; the first reads the raw conditioning, the others what the one in front stored activated
    act = None
    for i in range(int(c.voc_cond_layers)):
        _, act = eng.op_voc_conv1d(x if i == 0 else act, sd["condnet.%d.weight" % (2 * i)], sd["condnet.%d.bias" % (2 * i)], src_act=i > 0,
                                   act=ACT_ELU if i > 0 else ACT_NONE, want_raw=False, next_act=ACT_ELU, next_slope=1.0, stored=True)
        say("cond", i)
    # ReflectionPad1d(3) + Conv1d k7; its consumer is the first upsampler
    _, act = eng.op_voc_conv1d(act, sd["generator.1.weight"], sd["generator.1.bias"], reflect=True, src_act=True, act=ACT_ELU,
                               want_raw=False, next_act=ACT_LEAKY, next_slope=up_slope, stored=True)
    say("pre")
    cur = {"raw": None, "act": act, "f16": False}
    C, idx = int(c.voc_channels), 3
    for st in range(n_stages):
        s, depth = int(c.voc_scales[st]), int(c.voc_depth[st])
        C //= 2
        last_stage = st + 1 == n_stages
        kind, t16, _ = eng.plan_voc_stack(C, last_stage)
        # COPIED (vocoder.cpp act_form_ok): the 16-bit mode has an activated form for multiples of 64 channels only
        act_ok = p != 2 or C % 64 == 0
        # what the stack behind the upsampler reads
        if kind == "fused":
            needs_raw, needs_act, trunk16 = not t16, False, t16      # the raw trunk: one fp16 tensor, or fp32
        elif kind == "fused_wide" or act_ok:
            needs_raw, needs_act, trunk16 = not t16, True, False     # conv1 reads the activated trunk; the residual the raw one, if there is one
        else:
            needs_raw, needs_act, trunk16 = True, False, False
        src_act = cur["act"] is not None
        y, ya, up16 = eng.op_voc_upsample(cur["act"] if src_act else cur["raw"], sd["generator.%d.layer.weight" % idx],
                                          sd["generator.%d.layer.bias" % idx], s, up_slope=up_slope, src_act=src_act, want_raw=needs_raw,
                                          act_slope=1.0 if trunk16 else (res_slope if needs_act else None), stored=True)
        say("up", st, C, kind, t16, src_act, up16)
        if trunk16:     # fp16(y): the identity as activation
            cur = {"raw": ya.float(), "act": None, "f16": True}
        else:
            cur = {"raw": y, "act": ya, "f16": False}
        dil, li = 1, 0
        while li < depth:
            la = _layer(sd, idx + 1, li)
            if kind == "fused":
                pair = li + 1 < depth and eng.plan_voc_stack(C, last_stage, dil, dil * base)[2]
                lb = _layer(sd, idx + 1, li + 1) if pair else None
                last_layer = li + (2 if pair else 1) == depth
                # the fused kernels write an activated output in the 16-bit mode only (vfx_test.h: ya elsewhere is refused); the one
                # consumer that reads one is the upsampler behind the stack
                want_act = p == 2 and last_layer and not last_stage
                want_raw = not (t16 and want_act)      # fp16 trunk: nothing reads that layer's raw output; the fp32-trunk kernels always store y
                slope_out = up_slope if last_layer_slope is None else last_layer_slope
                y, ya, info = eng.op_voc_resblock_at(cur["raw"], None, la, dil, lb, dil * base if pair else 0, slope=res_slope,
                                                     act_slope=slope_out, last_stage=last_stage, want_raw=want_raw, want_act=want_act)
                assert bool(info["x16"]) == t16 and not info["asrc"], (st, li, info)
                say("fused", st, li, dil, pair, want_raw, want_act, info["rw"], info["r128"])
                cur = {"raw": y, "act": stored16(ya) if want_act else None, "f16": t16}
                if pair:
                    dil *= base
                    li += 1
            elif kind == "fused_wide":
                last_layer = li + 1 == depth
                want_act = not (last_layer and last_stage)     # the tail reads raw values
                slope_out = res_slope if not last_layer else (up_slope if last_layer_slope is None else last_layer_slope)
                y, ya, info = eng.op_voc_resblock_at(None if t16 else cur["raw"], cur["act"], la, dil, slope=res_slope, act_slope=slope_out,
                                                     last_stage=last_stage, want_raw=not t16, want_act=want_act)
                assert info["asrc"] and bool(info["x16"]) == t16, (st, li, info)
                say("wide", st, li, dil, t16, want_act)
                cur = {"raw": y, "act": stored16(ya) if want_act else None, "f16": False}
            elif act_ok:
                last_layer = li + 1 == depth
                _, h = eng.op_voc_conv1d(cur["act"], la[0], la[1], dil=dil, src_act=True, act=ACT_LEAKY, slope=res_slope, want_raw=False,
                                         next_act=ACT_LEAKY, next_slope=res_slope, stored=True)
                # raw: for the next layer's residual add (unless the activated fp16 trunk is the only form: t16) or for the tail
                want_raw = not t16 and (not last_layer or last_stage)
                to_tail = last_layer and last_stage
                slope_out = res_slope if not last_layer else (up_slope if last_layer_slope is None else last_layer_slope)
                y, ya = eng.op_voc_conv1d(h, la[2], la[3], src_act=True, act=ACT_LEAKY, slope=res_slope,
                                          residual=cur["act"] if t16 else cur["raw"], residual_act=t16, want_raw=want_raw,
                                          next_act=ACT_NONE if to_tail else ACT_LEAKY, next_slope=1.0 if to_tail else slope_out, stored=True)
                say("two", st, li, dil, t16, want_raw, to_tail)
                cur = {"raw": y, "act": ya, "f16": False}
            else:
                h, _ = eng.op_voc_conv1d(cur["raw"], la[0], la[1], dil=dil, act=ACT_LEAKY, slope=res_slope)
                y, _ = eng.op_voc_conv1d(h, la[2], la[3], act=ACT_LEAKY, slope=res_slope, residual=cur["raw"])
                say("two_raw", st, li, dil)
                cur = {"raw": y, "act": None, "f16": False}
            dil *= base
            li += 1
        idx += 3
    xt = cur["raw"]
    assert xt is not None, "the tail reads the raw trunk"
    if tail_activated:
        xt = torch.where(xt > 0, xt, xt * up_slope)
    w = sd["generator.%d.weight" % (idx + 1)]
    return eng.op_voc_final(xt, w, float(sd["generator.%d.bias" % (idx + 1)][0]), slope=up_slope, x_f16=cur["f16"])
