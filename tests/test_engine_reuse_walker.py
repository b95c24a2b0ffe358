"""No device: the inventory walker of tests/engine_reuse.py on a stand-in engine of CPU tensors, and the table helpers around it.  What the GPU
tests poison is what this walker finds: a buffer it misses is a buffer whose stale contents no test sees."""
import types

import torch

import engine_reuse as R
from ppmstereo_amd import _lib as L


def stand_in():
    e = types.SimpleNamespace()
    e.T, e.name, e.none = 3, "not a tensor", None
    e._FULL = torch.zeros(10, 2)
    e.VIEW = e._FULL[2:8]                                   # a view of another attribute: one storage, the owner's name
    e.SPT = L.SPTensor(6, 8, "cpu", before=2, after=3)      # halo rows belong to the buffer
    e.ALIAS = e.SPT                                         # XA is X
    e.NEST = [torch.zeros(3), [torch.zeros(4), (torch.zeros(5), "x")]]
    e.TABLE = {"a": torch.zeros(2), "b": {"c": L.SPTensor(2, 8, "cpu")}}
    e.EMPTY = torch.zeros(0)
    kept = torch.zeros(7)                                   # reachable through a launch object only
    e.ops = [("conv", types.SimpleNamespace(keep=[kept, e._FULL, e.SPT], ws=torch.zeros(16, dtype=torch.uint8), dev=torch.zeros(9, dtype=torch.uint8))),
             ("call", lambda: None)]
    e.chain = {"A": types.SimpleNamespace(keep=[kept], ws=None, cp=object())}
    e.timed = types.SimpleNamespace(fn=lambda: None, events=None)      # a TimedCall owns nothing
    return e, kept


def test_walker_finds_every_storage_once_under_the_owning_name():
    e, kept = stand_in()
    found = R.buffers(e)
    assert list(found) == ["_FULL", "SPT", "NEST[0]", "NEST[1][0]", "NEST[1][1][0]", "TABLE[a]", "TABLE[b][c]", "ops[0][1].ws", "ops[0][1].dev",
                           "ops[0][1].keep[0]"]
    assert found["_FULL"] is e._FULL and found["ops[0][1].keep[0]"] is kept
    assert found["SPT"] is e.SPT.data and tuple(found["SPT"].shape) == (2, 2 + 6 + 3, 8)             # before + own + after rows
    keys = [R.storage_key(t) for t in found.values()]
    assert len(set(keys)) == len(keys)
    assert sum(R.nbytes(t) for t in found.values()) == 80 + 352 + 12 + 16 + 20 + 8 + 64 + 16 + 9 + 28


def test_owner_comes_first_whatever_the_attribute_order():
    """An op list made before the buffers it keeps alive (the encoders' constructors): the attribute still owns the storage."""
    e = types.SimpleNamespace()
    buf = L.SPTensor(4, 8, "cpu")
    e.steps = [types.SimpleNamespace(keep=[buf], ws=None)]
    e.keep = [buf]
    e.s0 = buf
    assert list(R.buffers(e)) == ["s0"]


def test_table_lookup_and_check():
    table = {"pk.*": (R.CONST, None), "op[*].keep[*]": (R.CONST, "maybe"), "C1": (R.POISON, None), "C1[36:64]": (R.FINITE, None),
             "PRE[q1]": (R.POISON, "hoist"), "XT": (R.POISON, "attn"), "CF[0]": (R.POISON, None)}
    assert R.table_key(table, "pk.w[init0][2][0]") == "pk.*" and R.table_key(table, "op[fh1].keep[1]") == "op[*].keep[*]"
    assert R.table_key(table, "PRE[q1]") == "PRE[q1]" and R.table_key(table, "PRE[q2]") is None
    assert R.classify(table, "C1") == R.POISON and R.regions(table, "C1") == [(36, 64, R.FINITE)] and R.regions(table, "CF[0]") == []
    t = torch.zeros(1)
    found = {"pk.beta": t, "C1": t, "PRE[q1]": t, "CF[0]": t}
    assert R.check_table(table, found, have=("hoist",)) == []
    assert R.check_table(table, {**found, "NEW": t}, have=("hoist",)) == ["NEW: not in the table"]
    assert R.check_table(table, found, have=("attn",)) == ["PRE[q1]: found on an engine that should not have it", "XT: in the table, not found"]
    del found["C1"]
    assert R.check_table(table, found, have=("hoist",)) == ["C1: in the table, not found", "C1[36:64]: a region of a buffer that was not found"]


def test_every_engine_table_gives_each_name_one_class():
    for table in (R.SCALE_TABLE, R.FNET_TABLE, R.CNET_TABLE, R.SST_TABLE):
        for key, (cls, when) in table.items():
            assert cls in (R.CONST, R.POISON, R.FINITE, R.ZERO) and when in (None, "attn", "hoist", "maybe"), key
            if R.is_region(key):
                assert cls in (R.FINITE, R.ZERO) and table[key.split("[")[0]][0] == R.POISON, key
    assert all(R.classify(R.SCALE_TABLE, n) == R.POISON for n in R.SCALE_VALUES)


def test_poison_writes_each_class_its_value():
    e = types.SimpleNamespace(T=1, ksel=1, n=2)
    e.C1 = L.SPTensor(3, 64, "cpu", before=1)
    e.Z = torch.zeros(4, 2)
    e.PE = torch.ones(3)
    e.SEL = torch.zeros(4, 5, dtype=torch.int32)
    e._FLOW_full = torch.zeros(6, 2)
    e.ATT_WS = torch.zeros((260 + 2) * 4, dtype=torch.uint8)
    e.op = {"a": types.SimpleNamespace(ws=torch.zeros(10, dtype=torch.uint8), keep=[torch.ones(2)], dev=torch.ones(2, dtype=torch.uint8))}
    done = R.poison(e, R.SCALE_TABLE)
    assert set(done) == {"C1", "Z", "SEL", "_FLOW_full", "ATT_WS", "op[a].ws"}
    planes = e.C1.data.view(torch.int16)
    assert (planes[:, :, :36] == R.NAN16).all() and torch.isnan(e.C1.data[:, :, :36].float()).all()          # halo row included
    assert (e.C1.data[0, :, 36:].float() == 776.0).all() and (e.C1.data[1, :, 36:].float() != 0).all()         # (bf16 of 777) finite, lo not zero
    assert torch.isnan(e.Z).all() and (e.PE == 1).all() and (e.SEL == 3).all() and (e._FLOW_full == 1e9).all()
    words = e.ATT_WS.view(torch.int32)
    assert (words[:260] == R.NAN32).all() and (words[260:] == 1).all()
    ws = e.op["a"].ws
    assert (ws[:8].view(torch.int32) == R.NAN32).all() and (ws[8:] == 0xFF).all() and (e.op["a"].keep[0] == 1).all() and (e.op["a"].dev == 1).all()
