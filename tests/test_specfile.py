"""Schema descriptors from .spec text (spec_amd.specfile): field order, kinds, enums as int32,
list<message> as a NestedSchema, unsupported kinds (CPU)."""
from __future__ import annotations

import pytest

from spec_amd import Kind, NestedSchema, Schema
from spec_amd.specfile import load

SPEC = """
import ( "other" )
options ( go_package="example.com/x" )

enum Color {
    NONE = 0;
    RED = 1; // comment
}

// a record
message Record {
    id      bin128  1;
    seq     int64   2;
    name    string  3;
    color   Color   4;
    items   []Item  5;
}

message Item {
    key     int32   1;
    value   float64 2;
    label   string  3;
}

message Flat {
    a bool 1; b byte 2; c uint64 9; d bytes 10; e float32 11;
}

struct Pair { k int32; v int32; }

message WithStruct {
    p Pair 1;
    x int64 2;
}

service Svc {
    method(req Record 1) (resp Item 1);
}
"""


def test_flat_and_enum():
    f = load(SPEC)
    s = f.schema("Flat")
    assert isinstance(s, Schema)
    assert [(x.tag, x.kind) for x in s.fields] == [(1, Kind.BOOL), (2, Kind.BYTE), (9, Kind.UINT64),
                                                   (10, Kind.BYTES), (11, Kind.FLOAT32)]
    assert f.enums["Color"] == {"NONE": 0, "RED": 1}


def test_nested_record():
    s = load(SPEC).schema("Record")
    assert isinstance(s, NestedSchema)
    assert [(x.tag, x.kind) for x in s.outer.fields] == [(1, Kind.BIN128), (2, Kind.INT64), (3, Kind.STRING),
                                                         (4, Kind.INT32), (5, Kind.LIST)]
    assert [(x.tag, x.kind) for x in s.item.fields] == [(1, Kind.INT32), (2, Kind.FLOAT64), (3, Kind.STRING)]


def test_unsupported_kinds():
    f = load(SPEC)
    with pytest.raises(ValueError):
        f.schema("WithStruct")
    s = f.schema("WithStruct", skip_unsupported=True)
    assert [(x.tag, x.kind) for x in s.fields] == [(2, Kind.INT64)]


# ---- the full language (internal/lang/parser/grammar.y) and the reference's own schemas ----

import json  # noqa: E402
import os  # noqa: E402

from spec_amd import ListOf, Message, Struct  # noqa: E402
from spec_amd.specfile import SpecFile, load_files  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "spec_trees.json")

GRAMMAR = """
import (
    "pkg/a"
    b "pkg/bee"
)
options ( go_package="x/y/z" opt2="v" )

message Keywords {
    any     any         1;
    message message     2;
    struct  a.Thing     3;
    service []b.Item    4;
    options int32       5
}

struct S { import int16; oneway bool; }

service Svc {
    sub(id bin128 1) Sub;
    method();
    m0(msg string 1) oneway;
    m1(a int64 1, b float64 2, c bool 3) (a int64 1, b float64 2,);
    m2(Req) Resp;
    m3(a.Req) (<-In, Out->) Resp;
    m4(Req) (In<-) Resp;
    m5(Req) (->Out);
    m6() (<-[]In);
}

subservice Sub { hello(msg string 1) (msg string 1); }
"""


def test_grammar_constructs():
    f = SpecFile(GRAMMAR)
    assert f.package == "z" and f.imports == {"a": "pkg/a", "b": "pkg/bee"} and f.options["opt2"] == "v"
    assert f.messages["Keywords"] == [("any", "any", 1), ("message", "message", 2), ("struct", "a.Thing", 3),
                                      ("service", "[]b.Item", 4), ("options", "int32", 5)]
    assert f.structs["S"] == [("import", "int16"), ("oneway", "bool")]
    methods = {m[0]: m for m in f.services["Svc"]}
    assert methods["m0"][3] is True and methods["m2"][1:3] == ("Req", "Resp")
    assert methods["m3"][4] == {"in": "In", "out": "Out"} and methods["m3"][1] == "a.Req"
    assert methods["m4"][4] == {"in": "In"} and methods["m5"][4] == {"out": "Out"}
    assert methods["m6"][4] == {"in": "[]In"} and methods["sub"][2] == "Sub"
    assert methods["m1"][2] == [("a", "int64", 1), ("b", "float64", 2)]
    assert f.services["Sub"][0][0] == "hello"


def test_fixture_trees_shapes():
    d = json.load(open(GOLDEN))
    pkg1 = {f[0]: f for f in d["pkg1.Message"]}
    # struct1 Struct 61 -> STRUCT with int32 members; enum1 -> INT32; ints []int64 -> LIST<INT64>;
    # submessages1 []pkg2.Submessage -> LIST<MESSAGE> with pkg3a.Value struct; any -> ANY
    assert pkg1["struct1"][1:3] == [61, int(Kind.STRUCT)] and pkg1["struct1.key"][2] == int(Kind.INT32)
    assert pkg1["enum1"][2] == int(Kind.INT32) and pkg1["ints"][2:4] == [int(Kind.LIST), int(Kind.INT64)]
    assert pkg1["submessages1[].value.x"][2] == int(Kind.INT32) and pkg1["any"][2] == int(Kind.ANY)
    assert pkg1["message1"][2] == int(Kind.ANY)  # `message` = any message (Field(tag).Message())
    assert pkg1["submessage.next.value"][2] == int(Kind.STRING) and "submessage.next.next" not in pkg1
    mpx = {f[0]: f for f in d["pmpx.Message"]}
    assert mpx["code"][2] == int(Kind.INT32) and mpx["channel_open.id"][2] == int(Kind.BIN128)
    assert mpx["batch.list"][2:4] == [int(Kind.LIST), int(Kind.MESSAGE)]
    assert mpx["connect_request.versions"][2:4] == [int(Kind.LIST), int(Kind.INT32)]


def test_package_reference_trees_match_fixture():
    """build() precompiles the reference-derived trees from the package's own copy
    (spec_amd/data/reference_trees.json, no test-tree reads); it equals the golden fixture."""
    import json

    from spec_amd.tree_catalog import REFERENCE_TREE_NAMES, REFERENCE_TREES_JSON, reference_trees

    pkg = json.load(open(REFERENCE_TREES_JSON))
    gold = json.load(open(GOLDEN))
    assert sorted(pkg) == sorted(REFERENCE_TREE_NAMES)
    for k in REFERENCE_TREE_NAMES:
        assert pkg[k] == gold[k], k
    assert [t.to_fields() for t in reference_trees().values()] == \
        [[tuple(f) for f in gold[k]] for k in REFERENCE_TREE_NAMES]


def test_precompile_list_is_current():
    """build()'s list of test-only trees (tests/golden/precompile_trees.json, written by
    make_precompile_trees.py) holds exactly tests/trees.py's extra_trees(), so every tree the GPU
    tests decode has its kernels in the shipped code-object cache."""
    from spec_amd.tree_catalog import extra_trees as listed
    from tests.trees import extra_trees

    want = {k: t.to_fields() for k, t in extra_trees().items()}
    got = {k: t.to_fields() for k, t in listed().items()}
    assert got == want
