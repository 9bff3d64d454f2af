"""The bits join without a GPU: header against binding, a null handle, the Index refusals before the engine is touched."""
import ctypes as C
import re
import uuid
from pathlib import Path

import numpy as np
import pytest

from mlvectordb_amd import Index, Vector, _native
from tests.bits_range_helpers import BitsRangeOracleEngine

ROOT = Path(__file__).resolve().parents[1]
ENTRY = "mlvdb_join_within_bits"


def test_the_entry_is_declared_bound_and_refuses_a_null_handle():
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "mlvdb_bits_join.h").read_text(), flags=re.S)
    assert sorted(set(re.findall(r"\b(mlvdb_[a-z0-9_]+)\s*\(", text))) == [ENTRY] == sorted(_native.BITS_JOIN_SIGNATURES)
    params = [p.strip() for p in re.search(ENTRY + r"\((.*?)\);", text, flags=re.S).group(1).split(",")]
    restype, argtypes = _native.BITS_JOIN_SIGNATURES[ENTRY]
    assert len(params) == len(argtypes) == 16 and restype is C.c_int
    ctype_of = {"int64_t": C.c_int64, "int32_t": C.c_int32, "double": C.c_double}
    for p, ctype in zip(params, argtypes):
        want = (C.POINTER(_native.Where) if "mlvdb_where" in p else C.c_void_p) if "*" in p else ctype_of[p.split()[0]]
        assert ctype is want, p
    lib = _native.load()
    assert lib.mlvdb_abi_version() == 7 == _native.ABI_VERSION
    buf = (C.c_int64 * 4)()
    assert lib.mlvdb_join_within_bits(C.c_void_p(), 0, buf, 1, 0, 1, 0, 1.0, 1, 1, None, buf, buf, None, buf, buf) == 1
    assert b"null index handle" in lib.mlvdb_last_global_error()


class UntouchableEngine(BitsRangeOracleEngine):
    def join_within_bits(self, *a, **kw):
        raise AssertionError("the engine was touched")

    range_bits = search_bits = where_labels = bits_get = join_within_bits


def test_refusals_are_value_errors_before_the_engine_is_touched():
    rng = np.random.default_rng(2)
    index = Index(space="cosine", engine_factory=UntouchableEngine, attributes={"sig": "bits128", "year": "int"})
    vectors = [Vector(values=rng.standard_normal(4).astype(np.float32).tolist(),
                      metadata={"sig": rng.bytes(16), "year": i % 3}) for i in range(20)]
    index.add(vectors, "ns")
    ids, stranger = [v.id for v in vectors], uuid.uuid4()
    index.remove([ids[7]], "ns")
    sharded = Index(space="l2", devices=[0, 0], engine_factory=UntouchableEngine)
    for idx, args, kw, match in (
            (index, ("ns", "year", 3), {}, "needs a bits attribute"), (index, ("ns", "nope", 3), {}, "not a declared attribute"),
            (index, ("ns", "sig", 3), dict(metric="l2"), "metric must be one of"),
            (index, ("ns", "sig", float("nan")), {}, "radius must be a number"),
            (index, ("ns", "sig", 3), dict(where=lambda m: True), "one dict filter"),
            (index, ("ns", "sig", 3), dict(where={"nope": 1}), "not a declared attribute"),
            (index, ("ns", "sig", 3), dict(max_per_row=0), "max_per_row must be an int in"),
            (index, ("ns", "sig", 3), dict(max_per_row=16385), "max_per_row must be an int in"),
            (sharded, ("ns", "sig", 3), {}, "row-sharded")):
        for entry in (idx.join_within_bits, idx.duplicate_groups_bits):
            with pytest.raises(ValueError, match=match):
                entry(*args, **kw)
    for kw, match in ((dict(order="score"), "order must be one of"), (dict(ids=[ids[1], ids[1]]), "ids must not repeat"),
                      (dict(ids=[ids[1], stranger]), f"{stranger} is unknown or removed"),
                      (dict(ids=[ids[7]]), f"{ids[7]} is unknown or removed")):
        with pytest.raises(ValueError, match=match):
            index.join_within_bits("ns", "sig", 3, **kw)
    assert len(index.join_within_bits("other", "sig", 3)) == 0 and index.duplicate_groups_bits("other", "sig", 3) == []
