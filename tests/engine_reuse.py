"""What the engine re-use tests share (tests/test_engine_reuse_walker.py without a device, tests/test_gpu_engine_reuse.py with one): the inventory of
an engine's device buffers, the tables that give every buffer its class, the poison, and -- on the GPU side -- the clips, the dirtying sequence and
the state that is compared.

The property: what an engine holds after one clip cannot change the next clip.  A new engine is (almost) all zeros, so a launch that reads a buffer
before this clip wrote it reads 0 there and the previous clip's values on a used engine.  ``poison`` makes "the previous clip's values" the worst
ones that are still safe: NaN wherever a value stays a value, in-range wrong numbers wherever a value becomes an address.

Classes (one per table entry):
  CONST    never written after construction: packed weights, descriptors, parameter blocks, PE, the SST addend.  Not poisoned; bit-identical
           before and after a clip.
  POISON   everything a clip writes before it reads it -- what set_inp / set_net / set_flow / set_mhs / begin load included -- and what nothing reads.
  FINITE   a region no launch of a clip writes and some launch reads against zero weights: it must hold finite values, any finite values.
           Keys "NAME[c0:c1]": a channel range of an SP tensor whose other channels are POISON.  Poisoned with kernel_refs.JUNK.
  ZERO     a region that must hold zero.  None was found: the class exists so that a table can say it, and ``assert_zero`` checks it.
"""
import re

import torch

CONST, POISON, FINITE, ZERO = "CONST", "POISON", "FINITE", "ZERO"
JUNK = 777.0                                            # kernel_refs.JUNK: what padding that is never to matter holds
NAN16, NAN32 = 0x7FC0, 0x7FC00000                       # quiet NaN: one bf16 plane word, one fp32 word
FLOW_POISON = 1.0e9                                     # see SCALE_VALUES["_FLOW_full"]


# ------------------------------------------------------------------------------------------------ the inventory
def _is_sp(v):
    return hasattr(v, "data") and hasattr(v, "pixels") and hasattr(v, "channels") and torch.is_tensor(getattr(v, "data"))


def _is_launch(v):
    """A ConvOp / PwChain (or a stand-in): an object that owns a descriptor copy, a workspace or a keep list."""
    return not torch.is_tensor(v) and not _is_sp(v) and not isinstance(v, (list, tuple, dict, str, bytes)) and \
        any(hasattr(v, a) for a in ("ws", "keep")) and hasattr(v, "__dict__")


def _is_open(v):
    """Objects walked attribute by attribute: the packed weights of an update block."""
    return type(v).__name__ == "PackedBlock"


def storage_key(t):
    return t.untyped_storage().data_ptr()


def buffers(engine):
    """name -> tensor of every tensor reachable from ``engine``: its attributes (through lists, tuples and dicts), SPTensor.data (halo rows
    included), keep lists, and for every launch object (ConvOp, PwChain) in a container its ``ws``, ``dev`` and ``keep``.  One entry per storage,
    under the owning name: plain attributes first (in the order the constructor made them: _FLOW_full before its view FLOW, X before XA is X),
    then containers, then what only a launch object holds."""
    found, seen, launches = {}, set(), []

    def add(name, t):
        if t.numel() == 0:
            return
        k = storage_key(t)
        if k not in seen:
            seen.add(k)
            found[name] = t

    def walk(name, v):
        if torch.is_tensor(v):
            add(name, v)
        elif _is_sp(v):
            add(name, v.data)
        elif isinstance(v, (list, tuple)):
            for i, x in enumerate(v):
                walk(f"{name}[{i}]", x)
        elif isinstance(v, dict):
            for k, x in v.items():
                walk(f"{name}[{k}]", x)
        elif _is_open(v):
            for k, x in vars(v).items():
                walk(f"{name}.{k}", x)
        elif _is_launch(v):
            launches.append((name, v))

    attrs = list(vars(engine).items())
    for name, v in attrs:                               # owners: plain tensors and SP tensors
        if torch.is_tensor(v) or _is_sp(v):
            walk(name, v)
    for name, v in attrs:                               # containers (CF, Hb, PRE, X / Y of the SST engine, keep) and the packed weights
        if not (torch.is_tensor(v) or _is_sp(v)):
            walk(name, v)
    for name, op in launches:                           # what the launch objects own or keep alive
        for a in ("ws", "dev", "keep"):
            if getattr(op, a, None) is not None:
                walk(f"{name}.{a}", getattr(op, a))
    return found


def nbytes(t):
    return t.untyped_storage().nbytes()


# ------------------------------------------------------------------------------------------------ the tables
def _launch_entries(prefix):
    return {prefix + ".dev": (CONST, "maybe"),          # the descriptor / parameter block on the device: uploaded once
            prefix + ".keep[*]": (CONST, "maybe"),      # packed weights and biases that no PackedBlock attribute owns (the q/k pack, the encoders' packs)
            prefix + ".ws": (POISON, "maybe")}          # K-slice partials (fp32): the sliced launch writes every partial its reduce launch reads


# name -> (class, when): when None = on every engine of the class, "attn" = update_block16, "hoist" = update_block08 / 04, "maybe" = where it exists
SCALE_TABLE = {
    "pk.*": (CONST, None),                              # packed weights, shared between the engines of a block: one group
    "PE": (CONST, None),
    **_launch_entries("op[*]"), **_launch_entries("_qk_ops[*]"),
    # lookup writes all 64 channels (36 taps + zeros) and the flow copy X[254:256]; chain A reads CORR 64 wide
    "CORR": (POISON, None),
    "T1": (POISON, None),                               # no launch touches it
    # chain A stores its 36 real couts into C2; dw7 reads C2[0:40] and writes C1[0:40]: channels 36..39 meet all-zero depthwise weights and bias, but
    # the kernel adds its centre tap's input itself (x + dw(x)), so C1[36:40] = gelu(C2[36:40]): finite in, finite out.  Chain B reads C1 64 wide
    # against packs whose input rows 36..63 are zero ("channels beyond a layer's real inputs meet zero weights: they must hold finite values")
    "C2": (POISON, None), "C2[36:64]": (FINITE, None),  # reader: ppms_dwconv_gelu (dw7), channels 36..39; 40..63 nobody
    "C1": (POISON, None), "C1[36:64]": (FINITE, None),  # reader: ppms_pwchain (chain B), zero weight rows; 36..39 written from C2[36:40], 40..63 never
    "COR256": (POISON, None), "CF[0]": (POISON, None), "CF[1]": (POISON, None),
    "PATCH": (POISON, None),                            # flow_patch7 writes all 128 channels (98 taps + zeros)
    "FLO1": (POISON, None),
    # X = [inp | mf (126 couts of final_* + the lookup's flow copy at 254:256) | hid or mfg]: mem_attn writes both planes of X[256:384] (hid: an
    # all-zero lo plane, the promise behind lo_zero_from = 256) before any "_x" conv of the clip reads them
    "X": (POISON, None), "VAL": (POISON, None), "U1": (POISON, None),
    "XA": (POISON, "attn"), "XT": (POISON, "attn"), "MSG": (POISON, "attn"), "MSGN": (POISON, "attn"), "H1": (POISON, "attn"), "O1": (POISON, "attn"),
    "QKF": (POISON, "attn"), "VF": (POISON, "attn"), "M2": (POISON, "attn"), "M3": (POISON, "attn"), "KVWS": (POISON, "attn"),
    "Hb[0]": (POISON, None), "Hb[1]": (POISON, None), "Hb[2]": (POISON, None),
    "ZT": (POISON, None), "RT": (POISON, None), "RH": (POISON, None), "FH1": (POISON, None), "M1": (POISON, None),
    "Z": (POISON, None), "MASK": (POISON, None), "QK": (POISON, None),
    "_FLOW_full": (POISON, None),                       # (a coordinate: SCALE_VALUES)
    "_FH2Y_full": (POISON, None),                       # fh2 stores 54 of 64 columns; tap_gather_sum reads tap * 2 + c < 54 only: 54..63 nobody reads
    "DFLOW": (POISON, None),                            # tap_gather_sum writes columns 0, 1; get_dflow reads those two
    **{f"PRE[{k}]": (POISON, "hoist") for k in ("zr1_0", "q1", "zr2", "q2", "zr3", "q3")},
    "VT": (POISON, None), "QB": (POISON, None), "KB": (POISON, None),
    "ATT_WS": (POISON, None),                           # (partials and flag words: SCALE_VALUES)
    "UNC": (POISON, None), "PART": (POISON, None),
    "SIM": (POISON, None), "STRIVE": (POISON, None), "_STRIVE_next": (POISON, None), "SCORE": (POISON, None),
    "SEL": (POISON, None),                              # (a frame index: SCALE_VALUES)
    "SHAT": (POISON, None), "POOL": (POISON, None), "FLOW_OUT": (POISON, None),
    "_health": (POISON, "maybe"),                       # counters: a caller zeroes them (reset_attn_health) before it reads them
    "pyr[*]": (POISON, "maybe"),                        # the caller's correlation pyramid of the last begin(): the next begin() replaces it
}

FNET_TABLE = {
    **_launch_entries("ops[*][*]"),
    "stats": (POISON, None), "ws": (POISON, None), "s0": (POISON, None), "tout": (POISON, None), "out": (POISON, None), "keep[*]": (POISON, None),
}
CNET_TABLE = {
    **_launch_entries("steps[*]"),
    "stats": (POISON, None), "ws": (POISON, None), "s0": (POISON, None), "keep[*]": (POISON, None),
}
SST_TABLE = {
    **_launch_entries("steps[*]"),
    "addend": (CONST, None),
    "xin": (POISON, None), "X[*]": (POISON, None), "Y[*]": (POISON, None), "QF": (POISON, None), "KVF": (POISON, None), "M2": (POISON, None),
    "M3": (POISON, None), "MSG": (POISON, None), "MSGN": (POISON, None), "H1": (POISON, None), "O1": (POISON, None), "KVWS": (POISON, None),
}

# Buffers whose values become addresses (or decide which code runs): in-range wrong values, chosen after reading every reader.
#   SEL        int32 [Tg][5] frame indices.  Readers: ppms_attn_prep_k / pick_prep_k (row offset into the keys of frame sel), ppms_mem_attn (offset into
#              V^T of frame sel), forward_update_block's batched glue (gather).  All of them index with the value as it is: it must lie in [0, Tg).
#              Tg - 1 everywhere: in range, not what a new engine holds (0), and never a pick (the picks of a clip are distinct frames).
#   _FLOW_full fp32 flow: the lookup's sampling coordinate.  lookup_tap (corr_lookup.h) returns 0 for positions outside [-1, Wl] before it converts to
#              int; 1e9 is the value kernel_refs.lookup_inputs puts at pixel 9 of every lookup test.  Every other reader (flow_patch7, tap_gather_sum,
#              the upsamplings, f32_to_sp) uses the flow as a value.
#   ATT_WS     fp32 partials (O, m, l), then the 64-query kernel's int32 flag pairs.  Readers of a flag: the fix-up launch (mem_attn_kernel: != 0
#              means "recompute this tile", the tile's own index comes from the block id) and attn_redo_count_kernel (!= 0 is counted).  1 is the
#              value the kernel itself writes for a flagged tile; a stale 1 recomputes a tile on the other kernel and counts it: other bits, no address.
#   _health    int64 counters, only ever added to and read back.
SCALE_VALUES = ("SEL", "_FLOW_full", "ATT_WS", "_health")


def table_key(table, name):
    """The table key that covers a discovered name: the name itself, its form with every index replaced by *, or the group of its first
    component ("pk.*")."""
    if name in table:
        return name
    star = re.sub(r"\[[^\]]*\]", "[*]", name)
    if star in table:
        return star
    group = name.split(".", 1)[0].split("[", 1)[0] + ".*"
    return group if group in table else None


def classify(table, name):
    k = table_key(table, name)
    return None if k is None else table[k][0]


def regions(table, name):
    """[(c0, c1, class)] of the sub-regions "NAME[c0:c1]" the table lists for an SP tensor."""
    out = []
    for k, (cls, _) in table.items():
        m = re.fullmatch(re.escape(name) + r"\[(\d+):(\d+)\]", k)
        if m:
            out.append((int(m.group(1)), int(m.group(2)), cls))
    return out


def is_region(key):
    return re.fullmatch(r".*\[\d+:\d+\]", key) is not None


def check_table(table, found, have=()):
    """Every discovered name is in the table; every table name is discovered (entries marked "maybe" where they exist; "attn" / "hoist" where the
    engine is of that kind: ``have``).  -> the list of complaints."""
    bad = [f"{n}: not in the table" for n in found if table_key(table, n) is None]
    used = {table_key(table, n) for n in found}
    for k, (cls, when) in table.items():
        if is_region(k):
            if k.split("[")[0] not in found:
                bad.append(f"{k}: a region of a buffer that was not found")
        elif when == "maybe" or (when is not None and when not in have):
            if when not in (None, "maybe") and k in used:
                bad.append(f"{k}: found on an engine that should not have it")
        elif k not in used:
            bad.append(f"{k}: in the table, not found")
    return bad


# ------------------------------------------------------------------------------------------------ the poison
def _fill_nan(t):
    if t.dtype == torch.bfloat16 or t.dtype == torch.float16:
        t.view(torch.int16).fill_(NAN16)
    elif t.dtype == torch.float32:
        t.view(torch.int32).fill_(NAN32)
    elif t.dtype == torch.uint8:                        # a byte workspace of fp32 partials
        flat = t.reshape(-1)
        n4 = flat.numel() // 4 * 4
        flat[:n4].view(torch.int32).fill_(NAN32)
        flat[n4:].fill_(0xFF)
    else:
        raise TypeError(f"no NaN for {t.dtype}: an integer buffer needs a value of its own (SCALE_VALUES)")


def poison(engine, table):
    """Every buffer that is not CONST gets its class's poison, on the current stream.  The caller synchronises around it (the engines use side
    streams).  -> {name: class} of what was written."""
    done = {}
    for name, t in buffers(engine).items():
        cls = classify(table, name)
        assert cls is not None, f"{name}: not classified"
        if cls in (CONST, ZERO):
            continue
        if name == "SEL":
            t.fill_(t.shape[0] - 1)
        elif name == "_FLOW_full":
            t.fill_(FLOW_POISON)
        elif name == "_health":
            t.fill_(0x5A5A5A5A)
        elif name == "ATT_WS":
            words = t.view(torch.int32)
            partials = engine.T * engine.ksel * engine.n * 130
            words[:partials].fill_(NAN32)
            words[partials:].fill_(1)
        elif cls == FINITE:
            t.fill_(JUNK)
        else:
            _fill_nan(t)
        for c0, c1, rcls in regions(table, name):       # (2, rows, channels) planes of an SP tensor
            if rcls == FINITE:
                t[0, :, c0:c1] = JUNK
                t[1, :, c0:c1] = JUNK / 1024.0          # a lo plane that is not zero either
        done[name] = cls
    return done


def assert_zero(engine, table):
    for name, t in buffers(engine).items():
        if classify(table, name) == ZERO:
            assert not t.view(torch.int16 if t.element_size() == 2 else torch.int32).any(), f"{name} must stay all-zero"


# ------------------------------------------------------------------------------------------------ with a device: clips, the dirtying sequence, the state
DEV = "cuda:0"
BLOCKS = {"update_block16": 0, "update_block08": 1, "update_block04": 2}        # block -> its Attention_qk in model.att
STATE = ("up", "flow", "net", "mhs", "unc", "dflow", "mask", "SEL", "SHAT", "STRIVE", "SCORE", "KB", "VT")


def bits(t):
    t = t.contiguous()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def clip_inputs(T, h, w, seed, with_mhs, gain=1.0):
    from ppmstereo_amd.synth import synth_scale_inputs
    d = {k: (None if v is None else v.to(DEV)) for k, v in synth_scale_inputs(T, h, w, seed=seed, with_mhs=with_mhs, frame_contrast=1.0).items()}
    if gain != 1.0:
        d["fmap1"], d["fmap2"] = d["fmap1"] * gain, d["fmap2"] * gain
    return d


def load_clip(model, tag, eng, d, skip=()):
    """What forward_update_block does in front of the loop.  skip: loaders left out (the planted dependences of the can-fail test)."""
    from ppmstereo_amd.corr import CorrBlock1D
    dev = torch.device(DEV)
    if "set_inp" not in skip:
        eng.set_inp(d["inp"])
    if "set_net" not in skip:
        eng.set_net(d["net"])
    eng.set_flow(d["flow"])
    eng.set_mhs(d["mhs"])
    eng.begin(CorrBlock1D(d["fmap1"], d["fmap2"]).levels, model.att[BLOCKS[tag]].packed(dev))


def state(eng, up):
    """The state compared after an iteration, as clones taken on the current stream."""
    got = [up.clone(), eng.get_flow(), eng.get_net(), eng.get_mhs(), eng.get_unc(), eng.get_dflow(), eng.get_mask(), eng.SEL.clone(), eng.SHAT.clone(),
           eng.STRIVE.clone(), eng.SCORE.clone(), eng.KB.clone(), eng.VT.clone()]
    return dict(zip(STATE, got))


def run_clip(model, tag, eng, d, iters=3, skip=()):
    """Clip ``d`` on ``eng``: the loaders, begin, ``iters`` full iterations -> the state after every one (+ the health counters, zeroed first)."""
    with torch.cuda.device(torch.device(DEV)):
        eng.enable_attn_health(True)
        eng.reset_attn_health()
        load_clip(model, tag, eng, d, skip)
        out = [state(eng, eng.iterate()) for _ in range(iters)]
        health = eng.attn_health()
        torch.cuda.synchronize()
    return out, health


def differences(got, want):
    """[(iteration, name)] of every state entry that differs, health counters included."""
    (gs, gh), (ws, wh) = got, want
    bad = [(i, k) for i, (g, w) in enumerate(zip(gs, ws)) for k in STATE if not same(g[k], w[k])]
    return bad + ([("health", gh, wh)] if gh != wh else [])


def dirty(model, tag, eng, T, h, w, seed, clip_a_has_mhs):
    """The dirtying sequence on ``eng`` (slot 0 of its geometry): clip B -- another seed, features x 3, with_mhs the opposite of clip A's, five
    iterations so that parity ends at 1, the last one without mask head and upsampling, the health accounting on -- and then the block's module-level
    methods on random fp32 tensors, with an mfg whose lo plane is not zero.  They run on the same engine (slot 0 of (T, h, w))."""
    from ppmstereo_amd.weights import hash_normal
    blk = getattr(model, tag)
    b = clip_inputs(T, h, w, seed, with_mhs=not clip_a_has_mhs, gain=3.0)
    with torch.cuda.device(torch.device(DEV)):
        eng.enable_attn_health(True)
        load_clip(model, tag, eng, b)
        for _ in range(4):
            eng.iterate()
        assert eng.iterate(need_up=False) is None and eng.parity == 1
        r = lambda c, s: hash_normal((T, c, h, w), seed * 100 + s).to(DEV)
        assert blk.engine(T, h, w, torch.device(DEV)) is eng, "the module-level methods must run on the engine under test"
        blk.get_motion_and_value(r(2, 1), r(36, 2), r(64, 3).relu(), r(128, 4).relu())
        blk.get_uncertainty(r(256, 5))
        mfg = r(128, 8) * 1.2345678                     # arbitrary fp32: hi + lo with a lo plane that is not zero
        blk.forward(r(128, 6).tanh(), r(128, 7).relu(), r(128, 9), mfg, t=T)
        assert not eng._x_hid and bits(eng.X.own()[1, :, 256:384]).any(), "the lo plane of X[256:384] was meant to be non-zero here"
        torch.cuda.synchronize()
