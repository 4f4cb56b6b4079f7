"""The steps MilvusService's entry points share, over fakes - no device, no library: the workspace cache (_workspace_for), the
mask lease (_leased_masks / _released), the grouping cache (_cached_grouping), and a snapshot of the public surface of the service
and of the ctypes layer's index and workspace classes (tests/golden/service_surface.json, recorded before these steps were shared)."""
import inspect
import json
import os
import threading
from collections import OrderedDict

import pytest

from rag_project_icd10_amd import _native
from rag_project_icd10_amd.services.milvus_service import MilvusService

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "service_surface.json")
WORKSPACE_CLASSES = ("IcdFusion", "IcdMmr", "IcdByRows", "IcdBoost")
KINDS = {"fusion": ("fusion", "max_total"), "mmr": ("mmr", "max_nq"), "byrows": ("byrows", "max_nq"), "boost": ("boost_workspace", "max_nq")}


class FakeHandle:
    """a handle as the caches see one: `closed`, and a workspace's size under the name its kind goes by"""

    def __init__(self, size=0, key="max_nq"):
        self.size, self.closed = size, False
        setattr(self, key, size)

    def close(self):
        self.closed = True


class FakeIndex:
    """an index as the caches see it: every workspace and grouping it makes is noted"""

    def __init__(self, max_nq=1000):
        self.max_nq, self.closed, self.made, self.groupings = max_nq, False, [], []

    def _make(self, kind, size):
        self.made.append((kind, size))
        return FakeHandle(size, "max_total" if kind == "fusion" else "max_nq")

    def fusion(self, max_total):
        return self._make("fusion", max_total)

    def mmr(self, max_nq=None):
        return self._make("mmr", max_nq)

    def byrows(self, max_nq=None):
        return self._make("byrows", max_nq)

    def boost_workspace(self, max_nq=None):
        return self._make("boost", max_nq)

    def grouping(self, group_of, *, max_nq=None):
        self.groupings.append((group_of, max_nq))
        return FakeHandle()


class FakeClient:
    generation = 1


class FakeMask:
    def __init__(self, transient):
        self.transient, self.closes = transient, 0

    def close(self):
        self.closes += 1


def service():
    ms = MilvusService.__new__(MilvusService)
    ms.client = FakeClient()
    ms._views_lock = threading.Lock()
    ms._views, ms._masks, ms._groupings, ms._max_groupings = OrderedDict(), OrderedDict(), OrderedDict(), 3
    ms._workspaces, ms._dev_columns, ms._sparse = {}, None, None
    return ms


# ---- _workspace_for ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_workspace_cache_hits_and_rebuilds(kind):
    ms, index = service(), FakeIndex()
    ws = ms._workspace_for(kind, index, 100)
    assert index.made == [(kind, 100)] and ws.size == 100
    for need in (100, 99, 1):
        assert ms._workspace_for(kind, index, need) is ws                  # same index, same generation, room enough: nothing is built
    assert index.made == [(kind, 100)]
    grown = ms._workspace_for(kind, index, 101)                            # short
    assert grown is not ws and index.made[-1] == (kind, 101) and ms._workspace_for(kind, index, 100) is grown
    ms.client.generation = 2                                               # the store moved on
    moved = ms._workspace_for(kind, index, 10)
    assert moved is not grown and index.made[-1] == (kind, 64) and ms._workspace_for(kind, index, 64) is moved
    moved.close()                                                          # the handle was closed
    again = ms._workspace_for(kind, index, 10)
    assert again is not moved and len(index.made) == 4 and ms._workspace_for(kind, index, 10) is again
    other = FakeIndex()                                                    # another index object
    theirs = ms._workspace_for(kind, other, 10)
    assert theirs is not again and other.made == [(kind, 64)] and len(index.made) == 4
    assert ms._workspace_for(kind, index, 10) is not theirs and len(index.made) == 5      # ... and back: one entry per kind
    index.closed = True                                                    # the index was closed
    ms._workspace_for(kind, index, 10)
    assert len(index.made) == 6
    assert ms._workspaces[kind][0] is index and ms._workspaces[kind][2:] == (2,)


def test_workspace_size_asked_of_the_factory():
    for kind in KINDS:
        ms, index = service(), FakeIndex(max_nq=1000)
        for need, size in ((1, 64), (64, 64), (65, 65), (1001, 1000)):     # min(index.max_nq, max(need, 64))
            ms._workspaces.clear()
            assert ms._workspace_for(kind, index, need).size == size and index.made[-1] == (kind, size)
        assert type(index.made[-1][1]) is int
    assert MilvusService._WORKSPACES == KINDS


def test_workspace_kinds_do_not_evict_each_other_and_clear_views_empties_the_cache():
    ms, index = service(), FakeIndex()
    held = {kind: ms._workspace_for(kind, index, 70) for kind in KINDS}
    assert len(index.made) == 4 and set(ms._workspaces) == set(KINDS)
    for kind in KINDS:
        assert ms._workspace_for(kind, index, 70) is held[kind]
    assert len(index.made) == 4
    ms._clear_views()
    assert ms._workspaces == {} and ms._groupings == OrderedDict() and ms._views == OrderedDict() and ms._masks == OrderedDict()
    assert ms._workspace_for("mmr", index, 70) is not held["mmr"] and len(index.made) == 5


def test_fusions_reports_the_fusion_entry():
    ms, index = service(), FakeIndex()
    assert ms.fusions() == []
    ms._workspace_for("mmr", index, 70)
    assert ms.fusions() == []                                              # another kind is not a fusion
    ws = ms._workspace_for("fusion", index, 70)
    ws.stats = lambda: {"max_total": 70, "bytes": 4096}
    assert ms.fusions() == [{"max_total": 70, "generation": 1, "bytes": 4096}]
    ws.close()
    assert ms.fusions() == []


# ---- the mask lease ---------------------------------------------------------------------------------------------------------------
def test_no_filter_leases_nothing():
    ms, calls = service(), []
    ms._masks_for = lambda index, flt, nq: calls.append((flt, nq))
    with ms._leased_masks(object(), None, 5) as masks:
        assert masks is None
    assert calls == []


def test_masks_are_released_once_whether_the_body_returns_or_raises():
    ms, index = service(), object()
    for fails in (False, True):
        own, cached = FakeMask(True), FakeMask(False)
        calls, released = [], []
        ms._masks_for = lambda idx, flt, nq: (calls.append((idx, flt, nq)), [own, None, cached, own])[1]
        real = MilvusService._release_masks
        ms._release_masks = lambda masks: (released.append(list(masks)), real(masks))[1]
        if fails:
            with pytest.raises(KeyError, match="the body"):
                with ms._leased_masks(index, ["a", None, "b", "a"], 4) as masks:
                    raise KeyError("the body")
        else:
            with ms._leased_masks(index, ["a", None, "b", "a"], 4) as masks:
                assert masks == [own, None, cached, own] and own.closes == 0
        assert calls == [(index, ["a", None, "b", "a"], 4)] and released == [[own, None, cached, own]]
        # _release_masks's own rule through the lease: the search's own mask is closed (once per entry that holds it), a cached one stays
        assert own.closes == 2 and cached.closes == 0


def test_a_mask_appended_inside_the_block_is_released_with_the_others():
    ms = service()
    first, late = FakeMask(True), FakeMask(True)
    made = [first]
    with ms._released(made) as masks:
        assert masks is made
        made.append(late)                                                  # (the all-rows mask of a boosted search)
    assert first.closes == 1 and late.closes == 1
    with ms._released(None) as masks:
        assert masks is None


def test_sync_helper_leaves_host_outputs_alone():
    class Index:
        @property
        def device(self):
            raise AssertionError("a host output needs no device")
    import numpy as np
    MilvusService._sync_if_device(Index(), np.zeros(3))


# ---- _cached_grouping -------------------------------------------------------------------------------------------------------------
def test_grouping_cache_is_least_recently_used():
    ms, index = service(), FakeIndex(max_nq=5000)
    made = []
    make = lambda tag: lambda: (made.append(tag), tag)[1]   # noqa: E731
    g = {key: ms._cached_grouping(key, index, make(key)) for key in ("a", "b", "c")}
    assert made == ["a", "b", "c"] and index.groupings == [("a", 2048), ("b", 2048), ("c", 2048)] and list(ms._groupings) == ["a", "b", "c"]
    assert ms._cached_grouping("a", index, make("a")) is g["a"] and made == ["a", "b", "c"]       # a hit builds nothing ...
    assert list(ms._groupings) == ["b", "c", "a"]                                                # ... and is now the most recent
    g["d"] = ms._cached_grouping("d", index, make("d"))                                          # the _max_groupings + 1st: the least recent goes
    assert list(ms._groupings) == ["c", "a", "d"] and made[-1] == "d"
    assert ms._cached_grouping("b", index, make("b")) is not g["b"] and list(ms._groupings) == ["a", "d", "b"]
    small = FakeIndex(max_nq=100)
    ms._cached_grouping("s", small, make("s"))
    assert small.groupings == [("s", 100)]                                                       # max_nq = min(the index's, 2048)


def test_grouping_cache_rebuilds_for_another_index_or_a_closed_handle():
    ms, index, other = service(), FakeIndex(), FakeIndex()
    first = ms._cached_grouping("k", index, lambda: "ids")
    assert ms._cached_grouping("k", index, lambda: pytest.fail("a hit builds nothing")) is first
    theirs = ms._cached_grouping("k", other, lambda: "other ids")                                # the same key, another index object
    assert theirs is not first and other.groupings == [("other ids", 1000)] and ms._groupings["k"] == (other, theirs)
    theirs.close()                                                                               # a closed handle
    again = ms._cached_grouping("k", other, lambda: "ids again")
    assert again is not theirs and len(other.groupings) == 2
    other.closed = True                                                                          # a closed index
    assert ms._cached_grouping("k", other, lambda: "once more") is not again and len(other.groupings) == 3


# ---- the public surface -------------------------------------------------------------------------------------------------------------
def surface(cls):
    """public name -> the signature of a callable, "property", or the repr of a constant"""
    out = {}
    for name in sorted(n for n in dir(cls) if not n.startswith("_")):
        member = inspect.getattr_static(cls, name)
        value = getattr(cls, name)
        out[name] = "property" if isinstance(member, property) else (str(inspect.signature(value)) if callable(value) else repr(value))
    return out


def surfaces():
    return {"MilvusService": surface(MilvusService), **{name: surface(getattr(_native, name)) for name in ("IcdIndex",) + WORKSPACE_CLASSES}}


def test_public_surface_is_the_recorded_one():
    with open(GOLDEN, encoding="utf-8") as f:
        want = json.load(f)
    got = surfaces()
    assert set(got) == set(want)
    for name in want:
        assert got[name] == want[name], name


def test_workspace_classes_keep_their_stats_keys_and_messages():
    keys = {"IcdFusion": {"max_total", "bytes"}, "IcdMmr": {"max_nq", "bytes"}, "IcdByRows": {"max_nq", "bytes"}, "IcdBoost": {"max_nq", "bytes"}}
    nouns = {"IcdFusion": "fusion", "IcdMmr": "mmr workspace", "IcdByRows": "by-rows workspace", "IcdBoost": "boost workspace"}
    prefixes = {"IcdFusion": "fusion", "IcdMmr": "mmr", "IcdByRows": "byrows", "IcdBoost": "boost"}

    class Lib:
        """the three entry points of one workspace kind: create hands out a handle, stats writes (size, 4096)"""
        def __init__(self, prefix):
            self.calls = []
            setattr(self, f"icd_{prefix}_create", self.create)
            setattr(self, f"icd_{prefix}_stats", self.stats)
            setattr(self, f"icd_{prefix}_destroy", lambda h: self.calls.append(("destroy", h.value)) or 0)

        def create(self, index_h, size, out):
            self.calls.append(("create", index_h, size))
            out._obj.value = 77
            return 0

        def stats(self, h, size, nbytes):
            size._obj.value, nbytes._obj.value = 123, 4096
            return 0

    class Index:
        device, _h = 3, "the index handle"

    assert [c.__name__ for c in _native._Workspace.__subclasses__()] == list(WORKSPACE_CLASSES)
    assert all("stats" not in vars(getattr(_native, n)) for n in WORKSPACE_CLASSES)      # one stats() serves the four
    for name in WORKSPACE_CLASSES:
        cls, index = getattr(_native, name), Index()
        index._lib = Lib(prefixes[name])
        ws = cls(index, 200)
        size_key = (keys[name] - {"bytes"}).pop()
        assert index._lib.calls == [("create", "the index handle", 200)] and not ws.closed
        assert getattr(ws, size_key) == 200 and type(getattr(ws, size_key)) is int
        assert vars(ws).get("device") == (3 if name == "IcdFusion" else None)             # (only the fusion ever carried its device)
        assert ws.stats() == {size_key: 123, "bytes": 4096} and set(ws.stats()) == keys[name]
        ws.close()
        ws.close()
        assert ws.closed and index._lib.calls[1:] == [("destroy", 77)]
        with pytest.raises(_native.IcdError, match=f"libicdsearch error -5: {nouns[name]} is closed"):
            ws.stats()
