"""Vector store + search. Drop-in for the reference's services/milvus_service.py with the Milvus
engine replaced by an HBM-resident index searched by hand-written HIP kernels (libicdsearch.so).

Same public surface and return shapes: search (:271-320), insert_records (:208-269),
get_collection_stats (:322-341), load_collection (:343-357), clear_collection (:359-371),
test_connection (:373-408), release_collection (:410-434), get_collection_load_state (:436-458),
disconnect (:460-498), get_memory_usage (:500-522), health_check (:524-549),
_calculate_level_weight (:550-558); attributes .config .collection_name .embedding_service
.dimension .client (read by main.py and tools/build_database.py).

`MILVUS_DB_PATH` names a directory holding the on-disk corpus (corpus_store.py) instead of a Milvus
Lite file. `MILVUS_MODE=remote` (a gRPC client of a Milvus server, :84-111) is out of scope and raises.
There is no CPU search path: without libicdsearch.so / an MI355X, loading the collection fails and
`search` returns [] exactly as the reference does on engine errors (:318-320).

Additive: `search_batch` (many queries per call, numpy or device tensors); a Milvus `filter` expression on `search` and
`search_batch` (services/filter_expr.py): the selection's rows become a VIEW of the index (_native.IcdIndex.view, built on the
device), cached per (normalised expression, store generation) with LRU eviction (`ICD_FILTER_VIEWS`, default 8). With
`filter_mode="mask"`, or a LIST of expressions (one per query of a `search_batch`), the selection becomes a ROW MASK instead
(_native.IcdIndex.rowmask: a bitset of n / 8 bytes tested inside the scan, `ICD_FILTER_MASKS`, default 256).
"""
from __future__ import annotations

import contextlib
import datetime
import functools
import logging
import os
import threading
from collections import OrderedDict
from typing import Any, Dict, List, Optional

import numpy as np

from ..corpus_store import CorpusStore
from . import boost_ranker, filter_expr, hybrid_search as hybrid, range_search, rank_of, recommend, sparse_text, wide_search

logger = logging.getLogger(__name__)

_OUTPUT_FIELDS = ("code", "preferred_zh", "has_complication", "main_code", "secondary_code", "level",
                  "parent_code", "category_path", "semantic_text")


class QueryIterator:
    """pymilvus's query_iterator surface (MilvusService.query_iterator): next() -> the following rows of a
    filter's selection in ascending id as `query`-shaped dicts ([] when exhausted or after `limit` rows), close(). The cursor is a
    rank offset into ONE row mask held for the iterator's life (None: every row): a page is one select_rows call, whatever its
    depth. The iterator pins the index and the store generation it started on: after a mutation of the store next() raises
    RuntimeError instead of paging through two different corpora."""

    def __init__(self, service, index, mask, batch_size: int, limit: int, fields, start: int, generation_of):
        self._service, self._index, self._mask = service, index, mask
        self._batch, self._left = batch_size, (None if limit == -1 else limit)
        self._fields, self._cursor = fields, start
        self._generation_of = generation_of
        self._generation = generation_of()
        self._done = index is None

    def next(self) -> List[Dict[str, Any]]:   # noqa: A003 (pymilvus's name)
        if self._done or (self._left is not None and self._left <= 0):
            self._done = True
            return []
        if self._generation_of() != self._generation or self._index.closed or (self._mask is not None and self._mask.closed):
            raise RuntimeError("the collection changed under the iterator: start a new query_iterator")
        want = self._batch if self._left is None else min(self._batch, self._left)
        ids, total, taken = self._index.select_rows([self._mask], want, self._cursor)
        got = int(taken[0])
        self._cursor += got
        if got < want or self._cursor >= int(total[0]):
            self._done = True
        if got == 0:
            return []
        if self._left is not None:
            self._left -= got
        return self._service._rows_to_dicts(ids[0, :got], self._fields)

    def close(self):
        self._done = True
        if self._mask is not None:
            self._service._release_masks([self._mask])   # (a TEXT_MATCH mask is the iterator's own; a cached one stays)
        self._index = self._mask = None


class MilvusService:
    def __init__(self, embedding_service=None):
        self.config = self._load_config()
        self.collection_name = self.config.get("milvus", {}).get("collection_name", "icd10")
        self.embedding_service = embedding_service
        self.dimension = self._get_vector_dimension()
        self.client: Optional[CorpusStore] = None
        self._index = None          # rag_project_icd10_amd._native.IcdIndex
        self._index_rows = 0
        self._row_tags = None
        self._index_gen = -1        # the store generation the index was built from
        # filtered search: (normalised expression, store generation) -> view of the index over the selected rows, least recently
        # used first. NER and search run on different threads: every access holds the lock. An evicted view is only dropped from
        # the cache: a search that still holds it keeps it alive, the last reference closes it.
        self._views: "OrderedDict[tuple, Any]" = OrderedDict()
        self._views_lock = threading.Lock()
        self._max_views = max(1, int(os.getenv("ICD_FILTER_VIEWS", "8")))
        # masked search: (normalised expression, store generation) -> (the index it belongs to, IcdRowMask), least recently used
        # first, under the same lock and dropped where the views are. An evicted mask is closed by its last reference (a batch
        # in flight, an iterator).
        self._masks: "OrderedDict[tuple, Any]" = OrderedDict()
        self._max_masks = max(1, int(os.getenv("ICD_FILTER_MASKS", "256")))
        # grouping search: (field, store generation, normalised filter or None) -> (the index or view it belongs to, IcdGrouping)
        self._groupings: "OrderedDict[tuple, Any]" = OrderedDict()
        self._max_groupings = max(1, int(os.getenv("ICD_GROUPINGS", "16")))
        # hybrid, MMR, boosted and by-ids search: kind (_WORKSPACES) -> (the index it belongs to, its workspace handle, store
        # generation); one handle per kind, regrown when a call needs more room, dropped where the views and masks are
        self._workspaces: Dict[str, Any] = {}
        self._code_rows = None     # ((store, generation, rows), code -> first row): similar_codes' lookup, rebuilt when the store moves on
        # sparse search: (the index it belongs to, IcdSparse, SparseTextIndex, field, store generation); built lazily, one handle
        self._sparse = None
        # filter programs: (the index they belong to, IcdColumns, the filter_expr.Columns they were made from)
        self._dev_columns = None
        self._columns = None       # filter_expr.Columns of the store generation they were built from (rebuilt when it moves on)
        self._connect()
        self._setup_collection()

    # ---- configuration (reference :21-55) -------------------------------------------------------------
    def _load_config(self) -> Dict[str, Any]:
        return {"milvus": {
            "mode": os.getenv("MILVUS_MODE", "local"),
            "host": os.getenv("MILVUS_HOST", "localhost"),
            "port": int(os.getenv("MILVUS_PORT", "19530")),
            "username": os.getenv("MILVUS_USERNAME", ""),
            "password": os.getenv("MILVUS_PASSWORD", ""),
            "db_name": os.getenv("MILVUS_DB_NAME", "default"),
            "db_path": os.getenv("MILVUS_DB_PATH", "./db/milvus_icd10.db"),
            "collection_name": os.getenv("MILVUS_COLLECTION_NAME", "icd10"),
            "index_type": "FLAT",
            "metric_type": "IP",
            "secure": os.getenv("MILVUS_SECURE", "false").lower() == "true",
            # knobs of this build
            "gpu_device": int(os.getenv("ICD_GPU_DEVICE", os.getenv("LOCAL_RANK", "0"))),
            "max_batch": int(os.getenv("ICD_GPU_MAX_BATCH", "16384")),
            "max_k": int(os.getenv("ICD_GPU_MAX_K", "100")),
        }}

    def _get_vector_dimension(self) -> int:
        if self.embedding_service:
            try:
                return len(self.embedding_service.encode_query("测试文本"))
            except Exception as exc:
                logger.warning("无法从嵌入服务获取维度: %s", exc)
        return 1024

    def _connect(self):
        cfg = self.config.get("milvus", {})
        mode = cfg.get("mode", "local")
        try:
            if mode == "local":
                path = cfg.get("db_path", "./db/milvus_icd10.db")
                os.makedirs(path, exist_ok=True)
                self.client = CorpusStore.open(path, self.collection_name, self.dimension)
            elif mode == "remote":
                raise ValueError("MILVUS_MODE=remote (client of a Milvus server) is not part of this build; use 'local'")
            else:
                raise ValueError(f"不支持的Milvus模式: {mode}，请使用 'local' 或 'remote'")
        except Exception as exc:
            logger.error("Milvus连接失败 (模式: %s): %s", mode, exc)
            raise

    def _setup_collection(self):
        if not self.client.exists():
            self._create_collection()
        self._load_collection_to_memory()

    def _create_collection(self):
        self.client.create()

    # ---- HBM residency -----------------------------------------------------------------------------------
    def _load_collection_to_memory(self):
        """Upload the corpus to HBM (the reference's load_collection, :137-161). An empty collection
        counts as loaded. Raises if the native library / GPU is unavailable."""
        n = self.client.count
        if n == 0:
            self._drop_index()
            self._loaded = True
            return
        if self._index is not None and self._index_rows == n and self._index_gen == self.client.generation:
            self._loaded = True
            return
        from .._native import IcdIndex
        self._drop_index()
        cfg = self.config["milvus"]
        self._index = IcdIndex(self.client.matrix(), self.client.levels(), device=cfg["gpu_device"],
                               max_nq=cfg["max_batch"], max_k=cfg["max_k"])
        self._index_rows = n
        self._index_gen = self.client.generation
        self._loaded = True

    def _drop_index(self):
        self._clear_views()
        if self._index is not None:
            self._index.close()
        self._index = None
        self._index_rows = 0
        self._index_gen = -1
        self._row_tags = None
        self._loaded = False

    def supports_device_rescoring(self) -> bool:
        """True when search_batch returns device tensors that icd_hier_rescore can take (an index in HBM on a GPU)"""
        try:
            import torch
            return torch.cuda.is_available() and self._ready_index() is not None
        except Exception:
            return False

    def row_tags(self):
        """uint8 [n] on the index's GPU: what the device-side hierarchical rescoring needs to know about each row's code
        (HierarchicalSimilarityService.row_tag); built on first use after a load."""
        index = self._ready_index()
        if index is None:
            raise RuntimeError(f"collection {self.collection_name} is empty or missing")
        if getattr(self, "_row_tags", None) is None or self._row_tags.numel() != self.client.count:
            import torch
            from .hierarchical_similarity_service import HierarchicalSimilarityService as H
            tags = np.fromiter((H.row_tag(r.get("code") or "") for r in self.client.records), dtype=np.uint8, count=self.client.count)
            self._row_tags = torch.from_numpy(tags).to(torch.device("cuda", self.config["milvus"]["gpu_device"]))
        return self._row_tags

    # ---- writes -------------------------------------------------------------------------------------------
    def insert_records(self, records: List[Dict[str, Any]], embeddings: List[np.ndarray]) -> bool:
        if len(records) != len(embeddings):
            raise ValueError("记录数量与向量数量不匹配")
        try:
            rows, vecs = [], []
            for i, rec in enumerate(records):
                secondary = rec.get("secondary_code")
                main = rec.get("main_code")
                vecs.append(embeddings[i].tolist())  # a plain list here fails like the reference (:231)
                rows.append({
                    "code": rec["code"],
                    "preferred_zh": rec.get("preferred_zh", ""),
                    "has_complication": rec.get("has_complication", False),
                    "main_code": "" if main is None else main,
                    "secondary_code": "" if secondary is None else secondary,
                    "level": rec.get("level", 1),
                    "parent_code": rec.get("parent_code", ""),
                    "category_path": rec.get("category_path", ""),
                    "semantic_text": rec.get("semantic_text", ""),
                })
            mat = np.asarray(vecs, dtype=np.float32)
            if mat.ndim != 2 or mat.shape[1] != self.dimension:
                raise ValueError(f"vector dimension {mat.shape} != {self.dimension}")
            self.client.append(rows, mat)
            self._clear_views()
            self._loaded = self._index is not None and self._index_rows == self.client.count
            return True
        except Exception as exc:
            logger.error("插入记录失败: %s", exc)
            return False

    # ---- search ---------------------------------------------------------------------------------------------
    def _ready_index(self):
        if self.client is None or not self.client.exists():
            return None
        if self._index is None or self._index_rows != self.client.count or self._index_gen != self.client.generation:
            self._load_collection_to_memory()
        return self._index

    def _live_index(self):
        """the store's ready index; None without a client or a collection"""
        return self._ready_index() if self.client is not None and self.client.exists() else None

    # ---- filtered search ------------------------------------------------------------------------------------------------
    def _clear_views(self):
        with self._views_lock:
            self._views.clear()
            self._groupings.clear()
            self._masks.clear()
            self._dev_columns = None
            self._workspaces.clear()
            self._sparse = None

    # kind -> (the IcdIndex method that makes one, the attribute of the handle that holds its size)
    _WORKSPACES = {"fusion": ("fusion", "max_total"), "mmr": ("mmr", "max_nq"), "boost": ("boost_workspace", "max_nq"), "byrows": ("byrows", "max_nq")}
    # kinds whose workspace is made by a function (index, size) of their own module, not by a method of the index: the same cache,
    # the same rule
    _WORKSPACE_FACTORIES = {"rankof": (rank_of.make_workspace, "max_nq"), "wide": (wide_search.make_workspace, "max_nq"),
                            "recommend": (recommend.make_workspace, "max_requests")}

    def _workspace_for(self, kind: str, index, need: int):
        """the cached workspace of `kind` of `index` (the store's, or a view) with room for `need` queries, ids or sub-lists: one per
        kind, kept while the index, the store generation and the handle hold and it is large enough, else made anew"""
        gen = self.client.generation
        make, size = self._WORKSPACES.get(kind) or self._WORKSPACE_FACTORIES[kind]
        make = getattr(index, make) if isinstance(make, str) else functools.partial(make, index)
        with self._views_lock:
            hit = self._workspaces.get(kind)
            if hit is not None and hit[0] is index and hit[2] == gen and not index.closed and not hit[1].closed and getattr(hit[1], size) >= need:
                return hit[1]
            ws = make(min(index.max_nq, max(int(need), 64)))
            self._workspaces[kind] = (index, ws, gen)
        return ws

    # ---- grouping search (Milvus group_by_field / group_size) -------------------------------------------------------------
    def _grouping(self, field: str, index, rows, filter_key):
        """(IcdGrouping, values) of `field` for `index` - the store's index, or the view of the filter whose normalised form is
        filter_key and whose rows are `rows` (the view then gets the parent's group ids restricted to them). Cached per
        (field, store generation, filter) and dropped where the views are."""
        ids, values = self._filter_columns().group_ids(field)
        return self._cached_grouping((field, self.client.generation, filter_key), index, lambda: ids if filter_key is None else ids[rows]), values

    def _cached_grouping(self, key, index, make):
        """the IcdGrouping of `index` cached under `key`, now the most recently used; a missing one - or one of another index, or a
        closed one - is built from make() (the group id of every row of `index`) and the least recently used ones are evicted"""
        with self._views_lock:
            hit = self._groupings.get(key)
            if hit is not None and hit[0] is index and not index.closed and not hit[1].closed:
                self._groupings.move_to_end(key)
                return hit[1]
            grouping = index.grouping(make(), max_nq=min(index.max_nq, 2048))
            self._groupings[key] = (index, grouping)
            while len(self._groupings) > self._max_groupings:
                self._groupings.popitem(last=False)
        return grouping

    def groupings(self) -> List[Dict[str, Any]]:
        """the cached groupings, least recently used first: field, filter (normalised, None: the whole store), groups, rows of the
        largest group, HBM bytes"""
        with self._views_lock:
            items = list(self._groupings.items())
        out = []
        for (field, gen, fkey), (index, grouping) in items:
            if grouping.closed:
                continue
            st = grouping.stats()
            out.append({"field": field, "filter": fkey, "generation": gen, "groups": int(st["groups"]),
                        "largest_group": int(st["largest_group"]), "bytes": int(st["bytes"])})
        return out

    _check_scorer = staticmethod(filter_expr.check_group_scorer)

    # ---- argument checks the entry points share: none needs a store or a device ------------------------------------------------
    @staticmethod
    def _int_in(v, lo=None, hi=None) -> bool:
        """True for an int or a numpy integer - never a bool - with lo <= v <= hi (a bound of None is open)"""
        return not isinstance(v, bool) and isinstance(v, (int, np.integer)) and (lo is None or v >= lo) and (hi is None or v <= hi)

    @staticmethod
    def _one_filter(filter, message: str):   # noqa: A002
        """ValueError(message) for a list of filters where an entry point takes one expression"""
        if isinstance(filter, (list, tuple)):
            raise ValueError(message)

    def _filter_list(self, filters):
        """the filters of a query / count / facet batch as _masks_for takes them (_query_expr each); ValueError when not a list"""
        if isinstance(filters, str) or not isinstance(filters, (list, tuple)):
            raise ValueError("filters: a list of filter expressions")
        return [self._query_expr(e) for e in filters]

    @staticmethod
    def _batch_size(query_vectors):
        """(shape, nq) of a batch [nq, dim] or of one vector; ValueError on any other rank"""
        shape = np.shape(query_vectors)
        if len(shape) not in (1, 2):
            raise ValueError("query_vectors: [nq, dim] (or one vector)")
        return shape, 1 if len(shape) == 1 else int(shape[0])

    def _search_grouped(self, index, rows, filter, query_vectors, top_k: int, field: str, group_size: int, group_scorer=None):   # noqa: A002
        """(adj, raw, ids, levels, group values' ids, values) of a grouped search on the store's index or a filter's view; with a
        group_scorer a seventh entry follows: (the winning groups' scores [nq, top_k], their ids)"""
        whole = filter is None or index is self._index
        grouping, values = self._grouping(field, index, rows, None if whole else filter_expr.compile(filter))
        if group_scorer is not None:
            adj, raw, ids, levels, groups, gsc, gid = index.search_grouped(query_vectors, int(top_k), int(group_size), grouping,
                                                                            scorer=group_scorer, group_scores=True)
            return adj, raw, ids, levels, groups, values, (gsc, gid)
        adj, raw, ids, levels, groups = index.search_grouped(query_vectors, int(top_k), int(group_size), grouping)
        return adj, raw, ids, levels, groups, values

    @staticmethod
    def _add_group_scores(hit_lists, field, values, gsc, gid):
        """metadata["group_score"] of every hit of a scored grouped search: the score its group ranked by"""
        host = lambda t: t.cpu().numpy() if hasattr(t, "cpu") else t   # noqa: E731
        for hits, sc, gi in zip(hit_lists, host(gsc), host(gid)):
            by_value = {values[int(g)].item(): float(v) for v, g in zip(sc, gi) if g >= 0}
            for hit in hits:
                hit["metadata"]["group_score"] = by_value[hit["metadata"][field]]
        return hit_lists

    # ---- embedding-list search (Milvus embedding lists, metric MAX_SIM) -----------------------------------
    LIST_SCORERS = ("sum", "mean")
    LIST_MAX_VECTORS = 64   # include/icd_search.h ICD_MAXSIM_MAX_T

    @staticmethod
    def _check_list_args(lists, top_k, group_by_field, filter, scorer):   # noqa: A002
        """the checks of an embedding-list search that need no store and no device; returns the lists as float32 [T, dim] arrays"""
        if not MilvusService._int_in(top_k, 1, filter_expr.MAX_GROUPED_HITS):
            raise ValueError(f"top_k={top_k!r}: must be an integer in 1 .. {filter_expr.MAX_GROUPED_HITS}")
        if group_by_field is not None:
            filter_expr.check_grouping(group_by_field, top_k, 1)
        if not isinstance(scorer, str) or scorer not in MilvusService.LIST_SCORERS:
            raise ValueError(f"scorer={scorer!r}: not one of {', '.join(MilvusService.LIST_SCORERS)}")
        if filter is not None:
            if not isinstance(filter, str):
                raise ValueError("filter: one expression for all lists (a filter goes through a view)")
            filter_expr.compile(filter)
        out = []
        for i, vectors in enumerate(lists):
            v = np.asarray(vectors, dtype=np.float32)
            if v.ndim != 2 or not 1 <= v.shape[0] <= MilvusService.LIST_MAX_VECTORS:
                raise ValueError(f"list {i} of shape {v.shape}: need [1 .. {MilvusService.LIST_MAX_VECTORS} vectors, dim]")
            if out and v.shape[1] != out[0].shape[1]:
                raise ValueError(f"list {i} has dim {v.shape[1]}, list 0 dim {out[0].shape[1]}")
            out.append(v)
        return out

    def _list_grouping(self, field, index, rows, filter_key):
        """(IcdGrouping, values) for an embedding-list search: _grouping's for a field; for None every row is its own group, whose
        id is the row's id in the store (values None). Cached and dropped where the groupings are."""
        if field is not None:
            return self._grouping(field, index, rows, filter_key)
        own = lambda: np.arange(index.n, dtype=np.int32) if filter_key is None else np.asarray(rows, np.int32)   # noqa: E731
        return self._cached_grouping((None, self.client.generation, filter_key), index, own), None

    def search_embedding_lists_batch(self, lists, top_k: int = 10, group_by_field: Optional[str] = None,
                                     filter: Optional[str] = None, scorer: str = "sum") -> List[List[Dict[str, Any]]]:   # noqa: A002
        """Milvus's embedding-list search under MAX_SIM, exact: every entry of `lists` is ONE query of 1 .. 64 vectors [T, dim] -
        the segments of a text - and a group of rows scores the sum (scorer "mean": the mean over the vectors that hit it) over
        the list's vectors of its best row's inner product. group_by_field: one of filter_expr.GROUP_FIELDS, or None - every row
        its own group: codes ranked by their summed similarity to all segments. filter: one expression for all lists (its view).
        Per list the top_k best groups, best first: {"group": the group's value (None: the row's code), "score": the aggregate,
        "matches": per vector of the list the group's best row under it - the usual hit dict with "segment" = the vector's
        index - or None where the vector has no hit in the group}. A bad argument raises ValueError."""
        vecs = self._check_list_args(lists, top_k, group_by_field, filter, scorer)
        if not vecs:
            return []
        if self.client is None or not self.client.exists():
            logger.error("集合 %s 不存在", self.collection_name)
            return [[] for _ in vecs]
        rows = None
        if filter is not None:
            index, rows = self._filtered_index(filter)
        else:
            index = self._ready_index()
        if index is None:
            return [[] for _ in vecs]
        whole = filter is None or index is self._index
        grouping, values = self._list_grouping(group_by_field, index, rows, None if whole else filter_expr.compile(filter))
        list_off = np.concatenate([[0], np.cumsum([len(v) for v in vecs])]).astype(np.int64)
        gsc, gid, msc, mid, mlv = index.search_lists(np.concatenate(vecs), list_off, int(top_k), grouping, scorer=scorer)
        recs = self.client.records
        out = []
        for li in range(len(vecs)):
            v0, v1 = int(list_off[li]), int(list_off[li + 1])
            groups = []
            for j in range(int(top_k)):
                g = int(gid[li, j])
                if g < 0:
                    break
                adj = [float(np.float64(msc[t, j]) * self._calculate_level_weight(int(mlv[t, j]))) for t in range(v0, v1)]
                matches = []
                for t in range(v0, v1):
                    hit = self._hits_to_dicts(adj[t - v0:t - v0 + 1], msc[t, j:j + 1], mid[t, j:j + 1])
                    matches.append(dict(hit[0], segment=t - v0) if hit else None)
                groups.append({"group": recs[g].get("code") if values is None else values[g].item(), "score": float(gsc[li, j]),
                               "matches": matches})
            out.append(groups)
        return out

    def search_embedding_list(self, vectors, top_k: int = 10, group_by_field: Optional[str] = None, filter: Optional[str] = None,   # noqa: A002
                              scorer: str = "sum") -> List[Dict[str, Any]]:
        """search_embedding_lists_batch for ONE list of vectors [T, dim]"""
        return self.search_embedding_lists_batch([vectors], top_k, group_by_field, filter, scorer)[0]

    def _filter_columns(self) -> "filter_expr.Columns":
        gen = self.client.generation
        cols = self._columns
        if cols is None or cols.generation != gen or cols.n != self.client.count:
            cols = filter_expr.Columns.from_records(self.client.records, gen)
            self._columns = cols
        return cols

    def filter_rows(self, expr: str) -> np.ndarray:
        """sorted int64 row ids (= hit ids) of the rows that satisfy the Milvus filter expression `expr` (services/filter_expr.py);
        raises ValueError on a bad expression"""
        filter_expr.compile(expr)
        if self.client is None or not self.client.exists():
            return np.zeros(0, np.int64)
        cols = self._filter_columns()
        if filter_expr.has_text_match(expr):   # (the host route of TEXT_MATCH: the sparse index's rows, built lazily as search_text does)
            _sp, tx, field = self._text_index()
            cols.set_text_matcher(field, tx.match_rows)
        return cols.select(expr)

    def _filtered_index(self, expr: str):
        """(index, rows) to search for `expr`: the index itself when every row is selected, None when none is, else the
        selection's view (cached per normalised expression and store generation). Raises ValueError on a bad expression."""
        key = filter_expr.compile(expr)
        index = self._ready_index()
        if index is None:
            return None, np.zeros(0, np.int64)
        rows = self.filter_rows(expr)
        if len(rows) == 0:
            return None, rows
        if len(rows) == index.n:
            return index, rows
        ck = (key, self.client.generation)
        with self._views_lock:
            view = self._views.get(ck)
            if view is not None and not view.closed:
                self._views.move_to_end(ck)
                return view, rows
            view = index.view(rows)
            self._views[ck] = view
            while len(self._views) > self._max_views:
                self._views.popitem(last=False)
        return view, rows

    def filter_views(self) -> List[Dict[str, Any]]:
        """the cached filter views, least recently used first: expression (normalised), rows, HBM bytes"""
        with self._views_lock:
            items = list(self._views.items())
        out = []
        for (key, gen), view in items:
            if view.closed:
                continue
            st = view.stats()
            out.append({"expression": key, "rows": int(st["n"]), "generation": gen,
                        "bytes": int(st["bytes_corpus_f32"] + st["bytes_corpus_f16"] + st["bytes_workspace"])})
        return out

    # ---- masked search (a filter as a bitset over the rows, per query) ---------------------------------------------------------
    FILTER_MODES = ("view", "mask")

    @staticmethod
    def _check_filter_args(filter, filter_mode, group_by_field, nq=None):   # noqa: A002
        """the checks of `filter` / `filter_mode` that need no store and no device: ValueError on a bad mode, a bad expression
        (also inside a list), a list whose length is not nq, a list or mask mode next to group_by_field. Returns True when the
        search takes the mask path."""
        if filter_mode not in MilvusService.FILTER_MODES:
            raise ValueError(f"filter_mode={filter_mode!r}: one of {MilvusService.FILTER_MODES}")
        per_query = isinstance(filter, (list, tuple))
        if per_query:
            if nq is None:
                raise ValueError("a list of filters needs a batch: one expression (or None) per query of search_batch")
            if len(filter) != nq:
                raise ValueError(f"filter holds {len(filter)} expressions for {nq} queries")
            for e in filter:
                if e is not None:
                    filter_expr.compile(e)
        elif filter is not None:
            filter_expr.compile(filter)
        masked = per_query or (filter is not None and filter_mode == "mask")
        if masked and group_by_field is not None:
            raise ValueError("a per-query filter list / filter_mode='mask' cannot be combined with group_by_field")
        return masked

    # ---- keyword match filters (TEXT_MATCH) ------------------------------------------------------------------
    TEXT_MATCH_ON_DEVICE = True   # False: every TEXT_MATCH expression takes the host route (tests compare the two routes' bits)

    def _sparse_index(self):
        """(IcdSparse, SparseTextIndex) over the store's sparse field: the cached index's field, "preferred_zh" before one is built"""
        return self.build_sparse_index(self._sparse[3] if self._sparse is not None else "preferred_zh")

    def _text_index(self):
        """(IcdSparse, SparseTextIndex, field) of the store's sparse index, built on the first TEXT_MATCH as search_text builds it"""
        field = self._sparse[3] if self._sparse is not None else "preferred_zh"
        sp, tx = self.build_sparse_index(field)
        return sp, tx, field

    def _match_masks(self, index, shapes):
        """The masks of a batch of device-shaped TEXT_MATCH expressions (filter_expr.text_match_shape: (S, field, terms, m) each) in
        ONE IcdIndex.match_masks call, S's cached mask as the base. They belong to the search they were made for: not cached (the
        text is the query's own words), released by whoever asked (mask.transient marks them)."""
        sp, tx, field = self._text_index()
        pairs, mm, bases = [], [], []
        for rest, f, terms, m in shapes:
            if f != field:
                raise ValueError(f"TEXT_MATCH: no sparse index on {f}: call build_sparse_index")
            known, _total = tx.match_terms(terms)
            pairs.append((known, known))
            mm.append(m)
            bases.append(None if rest is None else self._filter_mask(index, rest))
        q_off, q_terms, _ = sparse_text.csr_from_pairs(pairs)
        masks = index.match_masks(sp, q_off, q_terms, mm, bases if any(b is not None for b in bases) else None)
        for m_ in masks:
            m_.transient = True
        return masks

    @staticmethod
    def _release_masks(masks):
        """close the per-search masks of a finished search (the cached ones stay)"""
        for m_ in masks or ():
            if m_ is not None and getattr(m_, "transient", False):
                m_.close()

    @contextlib.contextmanager
    def _released(self, masks):
        """`masks` for the length of a block, released (_release_masks) when it ends, returned or raised. The list is read at
        the end: a mask appended to it meanwhile is released with the others."""
        try:
            yield masks
        finally:
            self._release_masks(masks)

    def _leased_masks(self, index, filter, nq: int):   # noqa: A002
        """with ... as masks: the masks of a call's filter (_masks_for; None for no filter), released when the block ends"""
        return self._released(None if filter is None else self._masks_for(index, filter, nq))

    @staticmethod
    def _sync_if_device(index, out):
        """wait for the index's device if `out` is a device tensor: the search's own masks are closed next, it has to have run"""
        if hasattr(out, "cpu"):
            import torch
            torch.cuda.synchronize(index.device)

    # ---- filter programs (any boolean shape on the device) ---------------------------------------------------
    FILTER_ON_DEVICE = True   # False: section 17's two shapes keep section 17's call, every other expression takes the host route (tests compare the routes' bits)

    def _device_columns(self, index):
        """(IcdColumns, filter_expr.Columns) of the store's index, uploaded on the first device-routed expression and dropped where
        the masks are; (None, cols) for a store whose columns do not fit int32"""
        cols = self._filter_columns()
        with self._views_lock:
            hit = self._dev_columns
            if hit is not None and hit[0] is index and hit[2] is cols and not index.closed and not hit[1].closed:
                return hit[1], cols
        table = cols.device_columns()
        if table is None:
            return None, cols
        dev = index.columns(table)
        with self._views_lock:
            self._dev_columns = (index, dev, cols)
        return dev, cols

    def _device_program(self, index, expr):
        """the device program of `expr` (filter_expr.device_program), or None for the host route: the switch is off, the
        expression holds a TEXT_MATCH while TEXT_MATCH_ON_DEVICE is off, or the tree does not fit"""
        if not self.FILTER_ON_DEVICE:
            return None
        text = None
        if filter_expr.has_text_match(expr):
            if not self.TEXT_MATCH_ON_DEVICE:
                return None
            _sp, tx, field = self._text_index()
            text = {field: tx}
        dev, cols = self._device_columns(index)
        return None if dev is None else filter_expr.device_program(expr, cols, text)

    def _program_masks(self, index, exprs, programs):
        """The masks of a batch of expressions with their device programs in ONE IcdIndex.filter_masks call. A scalar-only
        expression's mask enters the mask cache under its normalised key, as a host-made one does; a mask of an expression that
        holds a TEXT_MATCH belongs to the search it was made for (mask.transient, section 17's rule)."""
        dev, _cols = self._device_columns(index)
        text = [filter_expr.has_text_match(e) for e in exprs]
        sp = self._text_index()[0] if any(text) else None
        masks = index.filter_masks(dev, sp, *filter_expr.pack_programs(programs))
        for i, (m_, t) in enumerate(zip(masks, text)):
            if t:
                m_.transient = True
            elif m_.stats()["rows"] == index.n:   # (a selection of every row passes no mask and is not cached, as on the host route)
                m_.close()
                masks[i] = None
        with self._views_lock:
            for e, m_, t in zip(exprs, masks, text):
                if m_ is not None and not t:
                    self._masks[(filter_expr.compile(e), self.client.generation)] = (index, m_)
            while len(self._masks) > self._max_masks:
                self._masks.popitem(last=False)
        return masks

    def _cached_mask(self, index, key):
        with self._views_lock:
            hit = self._masks.get((key, self.client.generation))
            if hit is not None and hit[0] is index and not index.closed and not hit[1].closed:
                self._masks.move_to_end((key, self.client.generation))
                return hit[1]
        return None

    def _mask_route(self, index, expr):
        """where the mask of `expr` comes from - the ONE place that holds the order and the two switches: ("cached", mask),
        ("program", its device program: section 18), ("text", its shape: section 17's call, for what section 18 refuses) or
        ("host", None). An expression whose TEXT_MATCH runs on the device gets a mask of its own: the cache is asked only once the
        device has refused it."""
        key = filter_expr.compile(expr)
        own = self.TEXT_MATCH_ON_DEVICE and filter_expr.has_text_match(expr)
        hit = None if own else self._cached_mask(index, key)
        if hit is not None:
            return "cached", hit
        program = self._device_program(index, expr)
        if program is not None:
            return "program", program
        shape = filter_expr.text_match_shape(expr) if self.TEXT_MATCH_ON_DEVICE else None
        if shape is not None:
            return "text", shape
        hit = self._cached_mask(index, key) if own else None
        return ("host", None) if hit is None else ("cached", hit)

    def _host_mask(self, index, expr):
        """the host route: the selection's rows as a cached mask (None when every row is selected: not cached)"""
        rows = self.filter_rows(expr)
        if len(rows) == index.n:
            return None
        with self._views_lock:
            mask = index.rowmask(rows)
            self._masks[(filter_expr.compile(expr), self.client.generation)] = (index, mask)
            while len(self._masks) > self._max_masks:
                self._masks.popitem(last=False)
        return mask

    def _filter_mask(self, index, expr):
        """the row mask of `expr` on the store's index: None when the expression is None or selects every row, else the
        selection's IcdRowMask (the empty mask when nothing is selected), cached per (normalised expression, generation) unless
        it is the search's own (_mask_route). The one-expression case of _masks_for."""
        mask = self._masks_for(index, expr, 1)[0]
        if mask is not None:
            mask.stats()   # (one mask: its row count is read now, for the callers that ask whether it is empty)
        return mask

    def _masks_for(self, index, filter, nq: int):   # noqa: A002
        """one entry per query: None (unfiltered) or the expression's mask; equal expressions share one mask. ALL device programs
        of the batch are one filter_masks call (section 18), the text parts of ALL section-17 shapes one match_masks call."""
        exprs = list(filter) if isinstance(filter, (list, tuple)) else [filter] * nq
        seen: Dict[Any, Any] = {}
        batched: Dict[str, Dict[Any, Any]] = {"text": {}, "program": {}}   # route -> expression -> its shape / program
        for e in exprs:
            if e is None or e in seen or e in batched["text"] or e in batched["program"]:
                continue
            route, what = self._mask_route(index, e)
            if route in batched:
                batched[route][e] = what
            else:
                seen[e] = what if route == "cached" else self._host_mask(index, e)
        if batched["text"]:
            seen.update(zip(batched["text"], self._match_masks(index, list(batched["text"].values()))))
        if batched["program"]:
            seen.update(zip(batched["program"], self._program_masks(index, list(batched["program"]), list(batched["program"].values()))))
        return [None if e is None else seen[e] for e in exprs]

    def filter_masks(self) -> List[Dict[str, Any]]:
        """the cached filter masks, least recently used first: expression (normalised), rows, HBM bytes"""
        with self._views_lock:
            items = list(self._masks.items())
        out = []
        for (key, gen), (_index, mask) in items:
            if mask.closed:
                continue
            st = mask.stats()
            out.append({"expression": key, "rows": int(st["rows"]), "generation": gen, "bytes": int(st["bytes"])})
        return out

    # ---- scalar query (Milvus query / count(*) / get / query_iterator) ----------------------------------------
    # The calls of MilvusClient that carry no vector. The primary key is the store's row id - the `id` a search hit carries (the
    # reference's collection is auto-id); results come in ascending id. The filter goes through _mask_route like a masked search's;
    # what is left is an ordered select over the masks' bits, on the device (_native.IcdIndex.select_rows). These methods are
    # additive: the reference's "never raise out of search" rule is not extended to them - a bad argument raises ValueError.
    QUERY_WINDOW = 16384   # Milvus's offset + limit bound; _native.SELECT_MAX_LIMIT
    COUNT_FIELD = "count(*)"

    @staticmethod
    def _query_fields(output_fields):
        """the checked field list of a query: the nine stored fields and `id` by default; `vector` on request"""
        if output_fields is None:
            return list(_OUTPUT_FIELDS) + ["id"]
        if isinstance(output_fields, str) or not isinstance(output_fields, (list, tuple)):
            raise ValueError("output_fields: a list of field names")
        fields = list(output_fields)
        for f in fields:
            if f not in _OUTPUT_FIELDS and f not in ("id", "vector"):
                raise ValueError(f"output_fields: unknown field {f!r}")
        if "id" not in fields:
            fields.append("id")   # (Milvus always returns the primary key)
        return fields

    @staticmethod
    def _query_expr(filter):   # noqa: A002
        """a query's filter as _masks_for takes it: None for no filter (also "" and blanks), else the checked expression"""
        if filter is None:
            return None
        if not isinstance(filter, str):
            raise ValueError("filter: a Milvus filter expression (a string)")
        if not filter.strip():
            return None
        filter_expr.compile(filter)   # (ValueError on a bad one, before anything is loaded)
        return filter

    @classmethod
    def _query_window(cls, limit, offset):
        for name, v, least in (("limit", limit, 1), ("offset", offset, 0)):
            if not cls._int_in(v, least):
                raise ValueError(f"{name}={v!r}: an int >= {least}")
        if int(offset) + int(limit) > cls.QUERY_WINDOW:
            raise ValueError(f"offset + limit = {int(offset) + int(limit)} exceeds {cls.QUERY_WINDOW}")
        return int(limit), int(offset)

    def _rows_to_dicts(self, ids, fields) -> List[Dict[str, Any]]:
        recs = self.client.records
        mat = self.client.matrix() if "vector" in fields else None
        out = []
        for i in ids:
            i = int(i)
            rec = recs[i]
            row = {}
            for f in fields:
                row[f] = i if f == "id" else (mat[i].tolist() if f == "vector" else rec.get(f))
            out.append(row)
        return out

    def _select_rows(self, index, masks, limit: int, offsets):
        """IcdIndex.select_rows over a batch of any length: max_nq masks per call"""
        nq, step = len(masks), index.max_nq
        if nq <= step:
            return index.select_rows(masks, limit, offsets)
        parts = [index.select_rows(masks[s:s + step], limit, offsets[s:s + step]) for s in range(0, nq, step)]
        return tuple(np.concatenate([p[i] for p in parts]) for i in range(3))

    def query_batch(self, filters, limit: int, offset=0, output_fields=None, with_totals: bool = False):
        """One `query` per entry of `filters` (an expression, "" or None each) with a shared limit and one offset for all or one per
        entry: a list of row lists. All masks come from ONE _masks_for call (one filter_masks launch for every device program of the
        batch, equal expressions share a mask), all rows from ONE select_rows call. with_totals: (lists, totals) - the number of
        rows every filter selects, counted by the same call."""
        exprs = self._filter_list(filters)
        nq = len(exprs)
        fields = self._query_fields(output_fields)
        offs = list(offset) if isinstance(offset, (list, tuple, np.ndarray)) else [offset] * nq
        if len(offs) != nq:
            raise ValueError(f"offset holds {len(offs)} entries for {nq} filters")
        offs = [self._query_window(limit, o)[1] for o in offs] if nq else []
        limit = self._query_window(limit, 0)[0]
        index = self._live_index()
        if index is None or nq == 0:
            return ([[] for _ in exprs], [0] * nq) if with_totals else [[] for _ in exprs]
        with self._leased_masks(index, exprs, nq) as masks:
            ids, total, taken = self._select_rows(index, masks, limit, np.asarray(offs, np.int64))
        lists = [self._rows_to_dicts(ids[q, :int(taken[q])], fields) for q in range(nq)]
        return (lists, [int(t) for t in total]) if with_totals else lists

    def count_batch(self, filters) -> List[int]:
        """the number of rows every filter of the list selects: one _masks_for call, one count pass over the masks"""
        exprs = self._filter_list(filters)
        index = self._live_index()
        if index is None or not exprs:
            return [0] * len(exprs)
        step = index.max_nq
        with self._leased_masks(index, exprs, len(exprs)) as masks:
            total = np.concatenate([index.count_rows(masks[s:s + step]) for s in range(0, len(masks), step)])
        return [int(t) for t in total]

    def count(self, filter: str = "") -> int:   # noqa: A002
        """Milvus's query(filter, output_fields=["count(*)"]) as a number"""
        return self.count_batch([filter])[0]

    # ---- facet counts (the terms aggregation over a filter's rows) ---------------------------------------------
    # How the rows a filter selects spread over the values of a field: the masks of _masks_for and the whole-store grouping of
    # _grouping, read together on the device (_native.IcdIndex.group_counts). Additive like the scalar query: bad arguments raise.
    @classmethod
    def _facet_args(cls, field, limit, min_count):
        if not isinstance(field, str) or field not in filter_expr.GROUP_FIELDS:
            raise ValueError(f"field={field!r}: not one of {', '.join(filter_expr.GROUP_FIELDS)}")
        if limit is not None and not cls._int_in(limit, 1):
            raise ValueError(f"limit={limit!r}: None or an int >= 1")
        if not cls._int_in(min_count, 0):
            raise ValueError(f"min_count={min_count!r}: an int >= 0")
        return None if limit is None else int(limit), int(min_count)

    def facet_batch(self, field: str, filters, limit: Optional[int] = None, min_count: int = 1, with_totals: bool = False):
        """One facet list per entry of `filters` (an expression, "" or None each): [{"value": v, "count": c}, ...] - the number of
        rows the filter selects under every value of `field` (one of filter_expr.GROUP_FIELDS), count descending, equal counts in
        the values' ascending order; values below min_count are left out, the list is cut at `limit` when one is given. All masks
        come from ONE _masks_for call (equal expressions share a mask, no filter is a NULL entry), all counts from one group_counts
        call per max_nq masks. with_totals: (lists, totals) - the rows every filter selects, the sum of its counts before the cut.
        An empty or unloaded collection answers []. Bad arguments raise ValueError."""
        limit, min_count = self._facet_args(field, limit, min_count)
        exprs = self._filter_list(filters)
        nq = len(exprs)
        index = self._live_index()
        if index is None or nq == 0:
            return ([[] for _ in exprs], [0] * nq) if with_totals else [[] for _ in exprs]
        grouping, values = self._grouping(field, index, None, None)
        step = index.max_nq
        with self._leased_masks(index, exprs, nq) as masks:
            counts = np.concatenate([index.group_counts(masks[s:s + step], grouping) for s in range(0, nq, step)])
        lists = []
        for row in counts:
            order = np.argsort(-row.astype(np.int64), kind="stable")   # (stable: equal counts keep the values' order)
            order = order[row[order] >= min_count][:limit]
            lists.append([{"value": values[j].item() if hasattr(values[j], "item") else values[j], "count": int(row[j])} for j in order])
        return (lists, [int(t) for t in counts.sum(axis=1, dtype=np.int64)]) if with_totals else lists

    def facet(self, field: str, filter: str = "", limit: Optional[int] = None, min_count: int = 1) -> List[Dict[str, Any]]:   # noqa: A002
        """the facet list of ONE filter (facet_batch)"""
        return self.facet_batch(field, [filter], limit, min_count)[0]

    def get(self, ids, output_fields=None) -> List[Dict[str, Any]]:
        """MilvusClient.get: the rows with these ids, in the order asked for; unknown ids are left out. Host only."""
        fields = self._query_fields(output_fields)
        if self._int_in(ids):
            ids = [ids]
        if isinstance(ids, (str, bytes)) or not isinstance(ids, (list, tuple, np.ndarray)):
            raise ValueError("ids: an int or a list of ints")
        for i in ids:
            if not self._int_in(i):
                raise ValueError(f"ids: {i!r} is not an int")
        if self.client is None or not self.client.exists():
            return []
        n = self.client.count
        return self._rows_to_dicts([int(i) for i in ids if 0 <= int(i) < n], fields)

    def query(self, filter: str = "", output_fields=None, limit: Optional[int] = None, offset: int = 0, ids=None) -> List[Dict[str, Any]]:   # noqa: A002
        """MilvusClient.query: the rows the filter selects, in ascending id, as dicts of output_fields (default: the nine stored
        fields and `id`; `vector` on request). output_fields=["count(*)"] gives [{"count(*)": total}] and takes neither limit nor
        offset, as in Milvus. limit=None: every matching row (walked in windows of 16384); else offset + limit <= 16384. ids=[...]
        without a filter is `get`. An empty or unloaded collection answers [] (a count of 0). Bad arguments raise ValueError."""
        expr = self._query_expr(filter)
        if ids is not None:
            if expr is not None:
                raise ValueError("query takes ids or a filter, not both")
            if limit is not None or offset != 0:
                raise ValueError("query by ids takes no limit and no offset")
            return self.get(ids, output_fields)
        if output_fields is not None and not isinstance(output_fields, str) and self.COUNT_FIELD in list(output_fields):
            if list(output_fields) != [self.COUNT_FIELD]:
                raise ValueError("count(*) cannot be combined with other output fields")
            if limit is not None or offset != 0:
                raise ValueError("count(*) takes no limit and no offset")
            return [{self.COUNT_FIELD: self.count(filter)}]
        if limit is not None:
            return self.query_batch([expr], limit, offset, output_fields)[0]
        fields = self._query_fields(output_fields)
        start = self._query_offset(offset)
        out: List[Dict[str, Any]] = []
        it = self.query_iterator(batch_size=self.QUERY_WINDOW, filter=filter, output_fields=fields, _start=start)
        try:
            while True:
                page = it.next()
                if not page:
                    return out
                out.extend(page)
        finally:
            it.close()

    @staticmethod
    def _query_offset(offset) -> int:
        if not MilvusService._int_in(offset, 0):
            raise ValueError(f"offset={offset!r}: an int >= 0")
        return int(offset)

    def query_iterator(self, batch_size: int = 1000, limit: int = -1, filter: str = "", output_fields=None, _start: int = 0) -> "QueryIterator":   # noqa: A002
        """pymilvus's query_iterator: an object whose next() returns the following batch_size rows of the filter's selection in
        ascending id ([] when exhausted or after `limit` rows), and close(). The cursor is a rank offset into ONE mask the iterator
        holds for its life; next() raises RuntimeError after the store changed, as search_iterator's does.
        batch_size <= 16384. Bad arguments raise ValueError."""
        expr = self._query_expr(filter)
        fields = self._query_fields(output_fields)
        if not self._int_in(batch_size, 1, self.QUERY_WINDOW):
            raise ValueError(f"batch_size={batch_size!r}: an int in 1 .. {self.QUERY_WINDOW}")
        if not self._int_in(limit, -1):
            raise ValueError("limit must be -1 (no limit) or a non-negative integer")
        index = self._live_index()
        mask = None if index is None or expr is None else self._masks_for(index, [expr], 1)[0]
        client = self.client
        return QueryIterator(self, index, mask, int(batch_size), int(limit), fields, int(_start),
                             lambda: (id(self.client), None if client is None else (client.generation, client.count)))

    @staticmethod
    def _check_band(top_k, group_by_field, radius, range_filter, offset, search_params):
        """(radius, range_filter, offset, banded) of a search's range arguments; ValueError on a bad one or on a combination with
        grouping (Milvus refuses that too)"""
        radius, range_filter = range_search.check_bounds(radius, range_filter, search_params)
        offset = range_search.check_offset(offset, top_k)
        banded = radius is not None or range_filter is not None or offset > 0
        if banded and group_by_field is not None:
            raise ValueError("radius / range_filter / offset cannot be combined with group_by_field")
        return radius, range_filter, offset, banded

    def search(self, query_vector: np.ndarray, top_k: int = 10, filter: Optional[str] = None,   # noqa: A002 (Milvus's name)
               group_by_field: Optional[str] = None, group_size: int = 1, radius: Optional[float] = None,
               range_filter: Optional[float] = None, offset: int = 0, search_params: Optional[Dict[str, Any]] = None,
               filter_mode: str = "view", group_scorer: Optional[str] = None) -> List[Dict[str, Any]]:
        """filter_mode: "view" (the default: the selection's cached view) or "mask" (the selection as a row mask of the index
        itself: no second index); the hits are the same. A bad value raises ValueError.
        group_by_field (one of filter_expr.GROUP_FIELDS) / group_size: Milvus's grouping search - the hits are the top_k best
        GROUPS' group_size best rows each (exact), re-sorted by adjusted score like any hit list; every hit's metadata then
        carries the group's value under the field's name. top_k * group_size <= 128. A bad grouping argument raises ValueError.
        group_scorer ("max", "sum" or "avg", next to group_by_field; Milvus's group scorer): what a group
        ranks by - its best row, or the sum / mean of its group_size best rows; every hit's metadata then also carries
        "group_score", that value of its group. Not given (None): a group ranks by its best row and no key is added.
        radius / range_filter (also search_params={"params": {"radius": .., "range_filter": ..}}): Milvus's range search - only
        rows with radius < inner product <= range_filter are ranked (the band is on the RAW score, `original_score`). offset: the
        hits of ranks offset .. offset + top_k of that ranking (offset + top_k <= 16384), then re-sorted by adjusted score. Exact
        (services/range_search.py). A bad range argument, or one next to group_by_field, raises ValueError."""
        if group_by_field is not None:
            filter_expr.check_grouping(group_by_field, top_k, group_size)
        elif group_size != 1:
            raise ValueError("group_size needs group_by_field")
        self._check_scorer(group_by_field, group_scorer)
        radius, range_filter, offset, banded = self._check_band(top_k, group_by_field, radius, range_filter, offset, search_params)
        if filter_mode not in self.FILTER_MODES:
            raise ValueError(f"filter_mode={filter_mode!r}: one of {self.FILTER_MODES}")
        self._one_filter(filter, "a list of filters needs a batch: one expression (or None) per query of search_batch")
        masked = filter is not None and filter_mode == "mask"   # (a bad expression is logged below and gives [], as on the view path)
        if masked and group_by_field is not None:
            raise ValueError("filter_mode='mask' cannot be combined with group_by_field")
        try:
            if self.client is None or not self.client.exists():
                logger.error("集合 %s 不存在", self.collection_name)
                return []
            rows = None
            if filter is not None and not masked:
                index, rows = self._filtered_index(filter)
            else:
                index = self._ready_index()
            if index is None:
                return []
            # (the reference sends data=[query_vector.tolist()], :282: a plain list has no .tolist and lands in the except below,
            #  an array's values arrive as float32 either way - converting through a Python list cost 35 us of a 130-us call)
            query_vector.tolist  # noqa: B018
            q = np.asarray(query_vector, dtype=np.float32).reshape(1, -1)
            band = (radius, range_filter, offset)
            if masked:
                out = self._search_masked(index, filter, 1, q, top_k, band)
            else:
                out = self._search_tail(index, rows, filter, q, top_k, group_by_field, group_size, group_scorer, band if banded else None)
            hits = self._hits_to_dicts(out[0][0], out[1][0], out[2][0], None if group_by_field is None else (group_by_field, out[4][0], out[5]))
            return hits if group_scorer is None else self._add_group_scores([hits], group_by_field, out[5], *out[6])[0]
        except Exception as exc:
            logger.error("搜索失败: %s", exc)
            return []

    def _search_masked(self, index, filter, nq: int, queries, top_k, band):   # noqa: A002
        """the masked branch of `search` and `search_batch`: the filter's masks leased around ONE search of the (index, masks) pair
        under band = (radius, range_filter, offset) -> (adj, raw, ids, levels)"""
        with self._leased_masks(index, filter, nq) as masks:   # (closing a mask synchronises the device: the search has run)
            return range_search.search_band((index, masks), queries, int(top_k), *band)

    def _search_tail(self, index, rows, filter, queries, top_k, group_by_field, group_size, group_scorer, band):   # noqa: A002
        """what `search` and `search_batch` run on the store's index or on a filter's view (`rows`: the view's): the grouped search
        (_search_grouped's tuple, scored with a group_scorer), the banded one (band = (radius, range_filter, offset), or None) or
        the plain one -> (adj, raw, ids, levels)"""
        if group_by_field is not None:
            return self._search_grouped(index, rows, filter, queries, top_k, group_by_field, group_size, group_scorer)
        if band is not None:
            return range_search.search_band(index, queries, int(top_k), *band)
        return index.search_reweighted(queries, int(top_k))

    def _hit_lists(self, adj, raw, ids, group=None, extra=None) -> List[List[Dict[str, Any]]]:
        """as_dicts of a batch: [nq, k] arrays (device tensors are moved to the host) -> one _hits_to_dicts list per query. group:
        None, or (field, the hits' group ids [nq, k], the field's values); extra: None, or (key, a float per hit [nq, k])"""
        host = lambda t: t.cpu().numpy() if hasattr(t, "cpu") else t   # noqa: E731
        adj, raw, ids = host(adj), host(raw), host(ids)
        if group is None:
            out = [self._hits_to_dicts(adj[q], raw[q], ids[q]) for q in range(len(ids))]
        else:
            groups = host(group[1])
            out = [self._hits_to_dicts(adj[q], raw[q], ids[q], (group[0], groups[q], group[2])) for q in range(len(ids))]
        if extra is not None:
            for hits, vals in zip(out, host(extra[1])):   # (padding sits behind the hits: the first len(hits) slots are theirs)
                for hit, v in zip(hits, vals):
                    hit[extra[0]] = float(v)
        return out

    def _hits_to_dicts(self, adj, raw, ids, group=None) -> List[Dict[str, Any]]:
        """group: None, or (field, the hits' group ids, the field's sorted distinct values) of a grouping search"""
        out = []
        recs = self.client.records
        for j, (a, r, i) in enumerate(zip(adj, raw, ids)):
            i = int(i)
            if i < 0:
                continue
            hit = recs[i]
            out.append({
                "code": hit.get("code"),
                "title": hit.get("preferred_zh"),
                "score": float(a),
                "original_score": float(r),
                "metadata": {
                    "has_complication": hit.get("has_complication", False),
                    "main_code": hit.get("main_code", ""),
                    "secondary_code": hit.get("secondary_code", ""),
                    "level": hit.get("level", 1),
                    "parent_code": hit.get("parent_code", ""),
                    "category_path": hit.get("category_path", ""),
                    "semantic_text": hit.get("semantic_text", ""),
                },
            })
            if group is not None:
                out[-1]["metadata"][group[0]] = group[2][int(group[1][j])].item()
        return out

    def search_iterator(self, query_vector, batch_size: int = 10, limit: int = -1, filter: Optional[str] = None,   # noqa: A002
                        radius: Optional[float] = None, range_filter: Optional[float] = None,
                        search_params: Optional[Dict[str, Any]] = None, filter_mode: str = "view") -> "range_search.SearchIterator":
        """pymilvus's search_iterator: an object whose next() returns the following batch_size hits of the query's ranking (inside
        the band, on the filter's selection) as a `search`-shaped list, [] when exhausted or after `limit` hits, and close().
        Pages are disjoint and exact at any depth; batch_size <= 128. The iterator keeps the index (or view) and the store
        generation it started on: next() raises RuntimeError after the store changed. Bad arguments raise ValueError.
        filter_mode="mask": the pages are those of the filter's row mask on the index itself (the same pages; the iterator keeps
        its own reference to the mask)."""
        radius, range_filter = range_search.check_bounds(radius, range_filter, search_params)
        self._one_filter(filter, "search_iterator takes one filter expression")
        masked = self._check_filter_args(filter, filter_mode, None)
        if self.client is None or not self.client.exists():
            index = None
        elif masked:
            index = self._ready_index()
            if index is not None:
                mask = self._filter_mask(index, filter)
                if mask is not None:
                    index = None if mask.rows == 0 else (index, mask)
        elif filter is not None:
            index, _ = self._filtered_index(filter)
        else:
            index = self._ready_index()
        client = self.client
        return range_search.SearchIterator(index, query_vector, batch_size, limit, radius, range_filter, self._hits_to_dicts,
                                           lambda: (id(self.client), None if client is None else (client.generation, client.count)))

    def search_batch(self, query_vectors, top_k: int = 10, as_dicts: bool = False, filter: Optional[str] = None,   # noqa: A002
                     group_by_field: Optional[str] = None, group_size: int = 1, radius: Optional[float] = None,
                     range_filter: Optional[float] = None, offset: int = 0, search_params: Optional[Dict[str, Any]] = None,
                     filter_mode: str = "view", group_scorer: Optional[str] = None):
        """Additive: many queries in one call. query_vectors: [nq, dim] numpy array or torch CUDA
        tensor. Returns (adjusted f64, raw f32, ids i64, levels i32), each [nq, top_k], in the order
        `search` returns hits; or, with as_dicts=True, a list of `search`-shaped hit lists.
        filter: a Milvus filter expression - only the rows it selects are ranked (hit ids stay the corpus's row ids); a selection
        shorter than top_k pads the lists with id -1, score -inf, level 0. Raises ValueError on a bad expression.
        filter may also be a list or tuple with ONE expression (or None: unfiltered) PER QUERY: every query is then ranked over its
        own selection in one call - row masks tested inside the scan, whatever filter_mode says. A length
        other than nq, a bad expression in it, or group_by_field next to it raise ValueError before anything is loaded. A query
        whose selection is empty comes back as padding ([] with as_dicts). filter_mode="mask" serves a single expression the same
        way, without a view; the default "view" is the cached view.
        group_by_field / group_size: as in `search`; the arrays are then [nq, top_k * group_size] and a fifth one follows, the
        hits' group ids (int32, -1 in padding: ranks of the field's sorted distinct values).
        group_scorer: as in `search`; two more arrays [nq, top_k] then follow in group-rank order, the winning groups' scores
        (float32, -inf in padding) and their ids (int32, -1 in padding); hit dicts carry metadata["group_score"].
        radius / range_filter / offset / search_params: as in `search`, the same band for every query of the batch; lists shorter
        than top_k are padded like a short filter selection's."""
        if group_by_field is not None:
            filter_expr.check_grouping(group_by_field, top_k, group_size)
        elif group_size != 1:
            raise ValueError("group_size needs group_by_field")
        self._check_scorer(group_by_field, group_scorer)
        radius, range_filter, offset, banded = self._check_band(top_k, group_by_field, radius, range_filter, offset, search_params)
        nq = None
        if isinstance(filter, (list, tuple)) or filter_mode != "view":   # (only the mask path counts the queries: the default path takes whatever it took)
            shape = np.shape(query_vectors)
            nq = 1 if len(shape) == 1 else int(shape[0])
        masked = self._check_filter_args(filter, filter_mode, group_by_field, nq)   # (a bad expression raises before anything is loaded)
        index = self._ready_index()
        if index is None:
            raise RuntimeError(f"collection {self.collection_name} is empty or missing")
        rows = None
        band = (radius, range_filter, offset)
        if masked:
            adj, raw, ids, levels = self._search_masked(index, filter, nq, query_vectors, top_k, band)
            return self._hit_lists(adj, raw, ids) if as_dicts else (adj, raw, ids, levels)
        if filter is not None:
            index, rows = self._filtered_index(filter)
            if index is None:   # nothing selected: no device call
                empty = self._empty_hits(query_vectors, int(top_k) * int(group_size), as_dicts)
                if group_by_field is None or as_dicts:
                    return empty
                if group_scorer is not None:
                    return empty + (empty[3] - 1, empty[1][:, :int(top_k)], (empty[3] - 1)[:, :int(top_k)])
                return empty + (empty[3] - 1,)
        # (large batches on a corpus of tight families of near-identical rows - ICD sibling codes - are handled inside the
        #  library: a second coarse pass over the queries the first could not certify, and from the next large batch on the
        #  wider partition right away; include/icd_search.h icd_stats.last_second_pass / wide_mode)
        out = self._search_tail(index, rows, filter, query_vectors, top_k, group_by_field, group_size, group_scorer, band if banded else None)
        if group_by_field is None:
            adj, raw, ids, levels = out
            return self._hit_lists(adj, raw, ids) if as_dicts else (adj, raw, ids, levels)
        adj, raw, ids, levels, groups, values = out[:6]
        scores = () if group_scorer is None else tuple(out[6])   # (gsc, gid) of a scored search
        if not as_dicts:
            return (adj, raw, ids, levels, groups) + scores
        lists = self._hit_lists(adj, raw, ids, (group_by_field, groups, values))
        return self._add_group_scores(lists, group_by_field, values, *scores) if scores else lists

    # ---- MMR search (a diverse top-k) ---------------------------------------------------------------------------
    MMR_MAX_FETCH = 128   # candidates per query (the hit list's slots)

    def _mmr_args(self, top_k, fetch_k, lambda_mult, radius, range_filter, search_params):
        """(top_k, fetch_k or None, lambda, radius, range_filter) checked without a store: ValueError on a bad one"""
        def whole(name, v):
            if not self._int_in(v):
                raise ValueError(f"{name}={v!r}: an int")
            return int(v)
        top_k = whole("top_k", top_k)
        if not 1 <= top_k <= self.MMR_MAX_FETCH:
            raise ValueError(f"top_k={top_k}: 1 .. {self.MMR_MAX_FETCH}")
        if fetch_k is not None:
            fetch_k = whole("fetch_k", fetch_k)
            if not top_k <= fetch_k <= self.MMR_MAX_FETCH:
                raise ValueError(f"fetch_k={fetch_k}: top_k={top_k} .. {self.MMR_MAX_FETCH}")
        if isinstance(lambda_mult, bool) or not isinstance(lambda_mult, (int, float, np.integer, np.floating)):
            raise ValueError(f"lambda_mult={lambda_mult!r}: a number in [0, 1]")
        lam = float(lambda_mult)
        if not 0.0 <= lam <= 1.0:   # (NaN fails both comparisons)
            raise ValueError(f"lambda_mult={lambda_mult!r}: a number in [0, 1]")
        radius, range_filter = range_search.check_bounds(radius, range_filter, search_params)
        return top_k, fetch_k, lam, radius, range_filter

    def search_mmr_batch(self, query_vectors, top_k: int = 10, fetch_k: Optional[int] = None, lambda_mult: float = 0.5,
                         filter=None, as_dicts: bool = False, radius: Optional[float] = None,   # noqa: A002
                         range_filter: Optional[float] = None, search_params: Optional[Dict[str, Any]] = None):
        """Additive: the top_k hits of every query that are not copies of each other - maximal marginal relevance over the query's
        fetch_k exact candidates, picked on the device (LangChain's max_marginal_relevance_search(query, k, fetch_k, lambda_mult);
        DESIGN.md section 21). lambda_mult in [0, 1]: 1 is plain relevance (`search` with filter_mode="mask"), 0 is diversity
        alone. fetch_k=None: min(128, the store's max k, max(20, 4 * top_k)). filter: one expression for the whole batch or a list
        with one entry (or None) per query, always as row masks of the index itself; radius / range_filter / search_params shape
        the candidate list as in `search`. Returns (adjusted f64, raw f32, ids i64, levels i32, mmr f64), each [nq, top_k], in
        adjusted-score order (level weight, one stable re-sort of the picked hits), padding id -1, -inf, level 0; with
        as_dicts=True a list of `search`-shaped hit lists whose hits carry "mmr_score", the value the hit was picked with.
        An empty or unloaded collection answers [] per query ([] hits each). Bad arguments raise ValueError."""
        top_k, fetch_k, lam, radius, range_filter = self._mmr_args(top_k, fetch_k, lambda_mult, radius, range_filter, search_params)
        shape, nq = self._batch_size(query_vectors)
        self._check_filter_args(filter, "mask", None, nq)   # (a bad expression raises before anything is loaded)
        index = self._live_index()
        if index is None:
            return [[] for _ in range(nq)]
        if shape[-1] != index.dim:
            raise ValueError(f"query dim {shape[-1]} != index dim {index.dim}")
        cap = min(self.MMR_MAX_FETCH, index.max_k)
        if fetch_k is None:
            fetch_k = min(cap, max(20, 4 * top_k))
        if fetch_k > cap or top_k > fetch_k:
            raise ValueError(f"top_k={top_k}, fetch_k={fetch_k}: need top_k <= fetch_k <= {cap} (the store's max k)")
        with self._leased_masks(index, filter, nq) as masks:
            adj, raw, ids, levels, mmr = index.search_mmr(query_vectors, top_k, fetch_k, lam, mmr=self._workspace_for("mmr", index, nq),
                                                          masks=masks, radius=radius, range_filter=range_filter, reweighted=True)
            if masks is not None:
                self._sync_if_device(index, adj)
        if not as_dicts:
            return adj, raw, ids, levels, mmr
        return self._hit_lists(adj, raw, ids, extra=("mmr_score", mmr))

    def search_mmr(self, query_vector, top_k: int = 10, fetch_k: Optional[int] = None, lambda_mult: float = 0.5,
                   filter: Optional[str] = None, radius: Optional[float] = None, range_filter: Optional[float] = None,   # noqa: A002
                   search_params: Optional[Dict[str, Any]] = None) -> List[Dict[str, Any]]:
        """the diverse hit list of ONE query (search_mmr_batch): `search`'s dicts in adjusted-score order, "mmr_score" added"""
        self._one_filter(filter, "a list of filters needs a batch: one expression (or None) per query of search_mmr_batch")
        q = np.asarray(query_vector, dtype=np.float32)
        if q.ndim != 1:
            raise ValueError("query_vector: one vector")
        return self.search_mmr_batch(q.reshape(1, -1), top_k, fetch_k, lambda_mult, filter=filter, as_dicts=True, radius=radius,
                                     range_filter=range_filter, search_params=search_params)[0]

    # ---- search by stored ids (Milvus 2.6's search by primary key) -------------------------------------------
    BY_IDS_MAX_K = 127   # the search runs at top_k + 1: the row's own hit takes a slot of the 128

    def _by_ids_args(self, top_k, include_self, radius, range_filter):
        """(top_k, radius, range_filter) checked without a store: ValueError on a bad one"""
        if not self._int_in(top_k):
            raise ValueError(f"top_k={top_k!r}: an int")
        top = self.BY_IDS_MAX_K + (1 if include_self else 0)
        if not 1 <= int(top_k) <= top:
            raise ValueError(f"top_k={top_k}: 1 .. {top}")
        radius, range_filter = range_search.check_bounds(radius, range_filter, None)
        return int(top_k), radius, range_filter

    @staticmethod
    def _id_list(ids) -> np.ndarray:
        if MilvusService._int_in(ids):
            ids = [ids]
        if isinstance(ids, (str, bytes)) or not isinstance(ids, (list, tuple, np.ndarray)):
            raise ValueError("ids: an int or a list of ints")
        arr = np.asarray(ids)
        if arr.ndim != 1 or (arr.size and (arr.dtype == bool or not np.issubdtype(arr.dtype, np.integer))):
            raise ValueError("ids: a flat list of ints")
        return np.ascontiguousarray(arr, np.int64)

    def _search_by_rows(self, index, rows, top_k, filter, nq, radius, range_filter, include_self):   # noqa: A002
        """one library call (chunked by the workspace) with the filter's masks taken and released around it"""
        with self._leased_masks(index, filter, nq) as masks:
            out = index.search_by_rows(rows, top_k, workspace=self._workspace_for("byrows", index, nq), masks=masks, radius=radius,
                                       range_filter=range_filter, include_self=include_self, reweighted=True)
            if masks is not None:
                self._sync_if_device(index, out[0])
        return out

    def search_by_ids(self, ids, top_k: int = 10, filter=None, radius: Optional[float] = None,   # noqa: A002
                      range_filter: Optional[float] = None, include_self: bool = False, as_dicts: bool = False):
        """Additive: Milvus 2.6's search by primary key - for every id the top_k rows closest to THAT STORED ROW, the row itself
        left out. The vectors never leave the device: the rows are gathered there, searched exactly at
        top_k + 1 and the row's own hit - which is not always the first: bit-identical rows tie and the smaller id leads - is cut
        out there. ids: an int or a list of row ids (the same id may repeat); an id the collection does not hold raises
        ValueError. filter: one expression for the whole batch or a list with one entry (or None) per id, always as row masks of
        the index itself; radius / range_filter as in `search`. include_self=True keeps the row's own hit (`search_batch` of the
        stored vectors with filter_mode="mask"). top_k: 1 .. 127 (128 with include_self), within the store's max k. Returns
        (adjusted f64, raw f32, ids i64, levels i32), each [len(ids), top_k], in the order `search` returns hits, padding id -1,
        -inf, level 0; with as_dicts=True a list of `search`-shaped hit lists. An empty or unloaded collection answers [] per
        id. Bad arguments raise ValueError."""
        top_k, radius, range_filter = self._by_ids_args(top_k, include_self, radius, range_filter)
        rows = self._id_list(ids)
        nq = int(rows.size)
        self._check_filter_args(filter, "mask", None, nq)   # (a bad expression raises before anything is loaded)
        index = self._live_index()
        if index is None:
            return [[] for _ in range(nq)]
        bad = rows[(rows < 0) | (rows >= index.n)]
        if bad.size:
            raise ValueError(f"ids: {int(bad[0])} is no row of the collection (0 .. {index.n - 1})")
        if top_k + (0 if include_self else 1) > index.max_k:
            raise ValueError(f"top_k={top_k}: the search runs at {top_k + (0 if include_self else 1)}, above the store's max k {index.max_k}")
        adj, raw, hit_ids, levels = self._search_by_rows(index, rows, top_k, filter, nq, radius, range_filter, include_self)
        if not as_dicts:
            return adj, raw, hit_ids, levels
        return self._hit_lists(adj, raw, hit_ids)

    def similar_codes(self, code: str, top_k: int = 10, filter: Optional[str] = None) -> List[Dict[str, Any]]:   # noqa: A002
        """the top_k codes closest to the stored record of `code` (search_by_ids of its row; of several records with the code, the
        first): `search`'s dicts, the record itself left out. KeyError when the collection holds no such code."""
        if not isinstance(code, str) or not code or '"' in code or "\\" in code:
            raise ValueError("code: a non-empty string without quotes or backslashes")
        self._one_filter(filter, "similar_codes takes one filter expression")
        top_k, _, _ = self._by_ids_args(top_k, False, None, None)
        self._check_filter_args(filter, "mask", None, 1)
        row = self._row_of_code(code)
        if row is None:
            raise KeyError(code)
        return self.search_by_ids([row], top_k, filter=filter, as_dicts=True)[0]

    def _row_of_code(self, code: str) -> Optional[int]:
        """the first row that carries `code`, from a dict built once per store generation (host only); None: no such code"""
        if self.client is None or not self.client.exists():
            return None
        gen = (id(self.client), self.client.generation, self.client.count)
        with self._views_lock:
            if self._code_rows is None or self._code_rows[0] != gen:
                table: Dict[str, int] = {}
                for i, rec in enumerate(self.client.records):
                    table.setdefault(rec.get("code"), i)
                self._code_rows = (gen, table)
            return self._code_rows[1].get(code)

    def knn_graph(self, top_k: int = 10, filter: Optional[str] = None, reweighted: bool = True):   # noqa: A002
        """Every row's top_k nearest other rows - a related-codes table, or the input of a near-duplicate sweep: (ids int64
        [n, top_k], scores float64 [n, top_k]) on the host, row r of both for the row of id r, padding id -1 and -inf. The ids
        are made on the device and walked in chunks of the workspace's max_nq; the host never holds a vector, only the two
        results come back. filter: ONE expression - every row's neighbours are taken among the rows it selects (a row outside it
        still gets neighbours). reweighted=True: `search`'s adjusted scores and order; False: the raw inner products, best
        first. An empty or unloaded collection answers two [0, top_k] arrays."""
        top_k, _, _ = self._by_ids_args(top_k, False, None, None)
        self._one_filter(filter, "knn_graph takes one filter expression")
        self._check_filter_args(filter, "mask", None, 1)
        index = self._live_index()
        if index is None:
            return np.zeros((0, top_k), np.int64), np.zeros((0, top_k), np.float64)
        if top_k + 1 > index.max_k:
            raise ValueError(f"top_k={top_k}: the search runs at {top_k + 1}, above the store's max k {index.max_k}")
        import torch
        n = int(index.n)
        ws = self._workspace_for("byrows", index, min(n, index.max_nq))
        step = min(ws.max_nq, index.max_nq)
        out_ids, out_scores = np.empty((n, top_k), np.int64), np.empty((n, top_k), np.float64)
        with self._leased_masks(index, filter, 1) as masks:
            mask = None if masks is None else masks[0]
            for r0 in range(0, n, step):
                rows = torch.arange(r0, min(n, r0 + step), dtype=torch.int64, device=torch.device("cuda", index.device))
                out = index.search_by_rows(rows, top_k, workspace=ws, masks=mask, reweighted=reweighted)
                scores, hit_ids = (out[0], out[2]) if reweighted else (out[0], out[1])
                out_ids[r0:r0 + len(rows)] = hit_ids.cpu().numpy()     # (the copy waits for the chunk: a mask is closed behind the loop)
                out_scores[r0:r0 + len(rows)] = scores.cpu().numpy()
        return out_ids, out_scores

    # ---- boosted search (Milvus 2.6's boost ranker) ----------------------------------------------------------
    def _boosted_index(self, index, rankers, filter, nq: int):   # noqa: A002
        """(the BoostedIndex of a batch, every mask it uses): the boost filters and the queries' own filters take ONE _masks_for
        call - device filter programs, TEXT_MATCH masks and the mask cache; equal expressions share a mask. A boost filter that
        selects every row still needs a mask (it rescales the whole ranking): the all-rows mask, made for this search."""
        boost_exprs = [r.filter for per in rankers for r in per]
        own = [] if filter is None else (list(filter) if isinstance(filter, (list, tuple)) else [filter] * nq)
        exprs = boost_exprs + own
        made = self._masks_for(index, exprs, len(exprs)) if exprs else []
        every = None
        pairs, at = [], 0
        for per in rankers:
            row = []
            for r in per:
                m_ = made[at]
                at += 1
                if m_ is None:
                    if every is None:
                        every = index.rowmask(np.arange(index.n, dtype=np.int64))
                        every.transient = True
                        made.append(every)
                    m_ = every
                row.append((m_, r.weight))
            pairs.append(row)
        masks = made[at:at + len(own)] if own else None
        return boost_ranker.BoostedIndex(index, self._workspace_for("boost", index, nq), pairs, masks), made

    def search_boosted_batch(self, query_vectors, top_k: int = 10, boosts=None, as_dicts: bool = False, filter=None,   # noqa: A002
                             radius: Optional[float] = None, range_filter: Optional[float] = None, offset: int = 0,
                             search_params: Optional[Dict[str, Any]] = None):
        """Additive: `search_batch` over the BOOSTED ranking - Milvus 2.6's boost ranker. boosts: ONE list of up to 4
        boost_ranker.BoostRanker (or {"filter", "weight"} dicts) for every query, or a list with one such list (or None) per
        query. The score of a row a ranker's filter selects is multiplied by its weight, in list order, BEFORE the top-k is chosen,
        exact over every row; `original_score` / the raw array carry the boosted score and the level reweight runs on it. filter:
        one expression for the batch or one (or None) per query, as row masks; it drops rows where a boost only re-ranks them.
        radius / range_filter / offset / search_params as in `search`, on the boosted score and ranking. Returns (adjusted f64,
        raw f32, ids i64, levels i32), each [nq, top_k], or with as_dicts=True `search`-shaped hit lists. An empty or unloaded
        collection answers [] per query. Bad arguments raise ValueError before anything is loaded."""
        shape, nq = self._batch_size(query_vectors)
        rankers = boost_ranker.rankers_per_query(boosts, nq)
        radius, range_filter, offset, _ = self._check_band(top_k, None, radius, range_filter, offset, search_params)
        if not self._int_in(top_k, 1, range_search.PAGE):
            raise ValueError(f"top_k={top_k!r}: 1 .. {range_search.PAGE}")
        self._check_filter_args(filter, "mask", None, nq)
        index = self._live_index()
        if index is None:
            return [[] for _ in range(nq)]
        if shape[-1] != index.dim:
            raise ValueError(f"query dim {shape[-1]} != index dim {index.dim}")
        bi, made = self._boosted_index(index, rankers, filter, nq)
        with self._released(made):
            adj, raw, ids, levels = range_search.search_band(bi, query_vectors, int(top_k), radius, range_filter, offset)
            self._sync_if_device(index, adj)
        if not as_dicts:
            return adj, raw, ids, levels
        return self._hit_lists(adj, raw, ids)

    def search_boosted(self, query_vector, top_k: int = 10, boosts=None, filter: Optional[str] = None,   # noqa: A002
                       radius: Optional[float] = None, range_filter: Optional[float] = None, offset: int = 0,
                       search_params: Optional[Dict[str, Any]] = None) -> List[Dict[str, Any]]:
        """the boosted hit list of ONE query (search_boosted_batch): `search`'s dicts, `original_score` the boosted score"""
        self._one_filter(filter, "a list of filters needs a batch: one expression (or None) per query of search_boosted_batch")
        q = np.asarray(query_vector, dtype=np.float32)
        if q.ndim != 1:
            raise ValueError("query_vector: one vector")
        if boosts is not None and any(b is None or isinstance(b, (list, tuple)) for b in (boosts if isinstance(boosts, (list, tuple)) else ())):
            raise ValueError("boosts: one list of BoostRanker for the one query")
        return self.search_boosted_batch(q.reshape(1, -1), top_k, boosts, as_dicts=True, filter=filter, radius=radius,
                                         range_filter=range_filter, offset=offset, search_params=search_params)[0]

    def search_boosted_iterator(self, query_vector, boosts=None, batch_size: int = 10, limit: int = -1, filter: Optional[str] = None,   # noqa: A002
                                radius: Optional[float] = None, range_filter: Optional[float] = None,
                                search_params: Optional[Dict[str, Any]] = None) -> "range_search.SearchIterator":
        """`search_iterator` over the boosted ranking of one query: next() returns the following batch_size hits of it (inside the
        band, on the filter's selection), pages disjoint and exact at any depth - the cursor is a boosted score and an id. The
        iterator keeps its masks and the store generation it started on."""
        radius, range_filter = range_search.check_bounds(radius, range_filter, search_params)
        self._one_filter(filter, "search_boosted_iterator takes one filter expression")
        rankers = boost_ranker.rankers_per_query(boosts, 1)
        self._check_filter_args(filter, "mask", None, 1)
        index = self._live_index()
        range_search.SearchIterator(None if index is None else index, query_vector, batch_size, limit, radius, range_filter, None,
                                    lambda: None).close()   # (its argument checks, before a mask is made)
        bi = None if index is None else self._boosted_index(index, rankers, filter, 1)[0]
        client = self.client
        return range_search.SearchIterator(bi, query_vector, batch_size, limit, radius, range_filter, self._hits_to_dicts,
                                           lambda: (id(self.client), None if client is None else (client.generation, client.count)))

    # ---- hybrid search (Milvus hybrid_search over dense requests) ------------------------------------------
    def fusions(self) -> List[Dict[str, Any]]:
        """the cached hybrid-search workspace (at most one): sub-lists per call, HBM bytes"""
        with self._views_lock:
            hit = self._workspaces.get("fusion")
        if hit is None or hit[1].closed:
            return []
        st = hit[1].stats()
        return [{"max_total": int(st["max_total"]), "generation": hit[2], "bytes": int(st["bytes"])}]

    # ---- sparse search (BM25 over a text field) ---------------------------------------------------------------
    SPARSE_MAX_NQ = 1024   # queries per icd_sparse_search call (longer batches are sent in pieces)

    def build_sparse_index(self, field: str = "preferred_zh"):
        """(IcdSparse, SparseTextIndex) over `field` of the store's records: analyzer + BM25 on the host, postings on the device.
        Built lazily, cached per store generation and field, dropped where the views, masks and fusions are."""
        index = self._ready_index()
        if index is None:
            raise RuntimeError(f"collection {self.collection_name} is empty or missing")
        gen = self.client.generation
        with self._views_lock:
            hit = self._sparse
            if hit is not None and hit[0] is index and hit[3] == field and hit[4] == gen and not index.closed and not hit[1].closed:
                return hit[1], hit[2]
        recs = self.client.records
        if recs and field not in recs[0]:
            raise ValueError(f"field={field!r}: not a field of the store's records")
        tx = sparse_text.SparseTextIndex([str(r.get(field) or "") for r in recs])
        sp = index.sparse(tx.row_off, tx.terms, tx.vals, tx.vocab_size, max_nq=min(index.max_nq, self.SPARSE_MAX_NQ), max_k=index.max_k)
        with self._views_lock:
            self._sparse = (index, sp, tx, field, gen)
        return sp, tx

    def sparse_indexes(self) -> List[Dict[str, Any]]:
        """the cached sparse index (at most one): field, vocabulary, postings, HBM bytes"""
        with self._views_lock:
            hit = self._sparse
        if hit is None or hit[1].closed:
            return []
        st = hit[1].stats()
        return [{"field": hit[3], "vocab": int(st["vocab"]), "nnz": int(st["nnz"]), "generation": hit[4], "bytes": int(st["bytes"])}]

    def _sparse_lists(self, index, sp, q_off, q_terms, q_vals, k: int, masks, reweighted: bool, grouping=None, group_size: int = 1):
        """search_sparse over a batch of any length, SPARSE_MAX_NQ queries per call (fewer where the grouping of a grouped call
        holds fewer); host arrays in and out"""
        q_off = np.asarray(q_off, np.int64)
        nq = len(q_off) - 1
        step = sp.max_nq if grouping is None else min(sp.max_nq, grouping.max_nq)
        outs = []
        for s0 in range(0, max(nq, 1), step):
            s1 = min(nq, s0 + step)
            a, b = int(q_off[s0]), int(q_off[s1])
            outs.append(index.search_sparse(sp, q_off[s0:s1 + 1] - a, q_terms[a:b], q_vals[a:b], k,
                                            masks=None if masks is None else masks[s0:s1], reweighted=reweighted,
                                            grouping=grouping, group_size=group_size))
        return tuple(np.concatenate([o[i] for o in outs]) for i in range(len(outs[0])))

    def search_sparse_batch(self, q_off, q_terms, q_vals, top_k: int = 10, filter=None, as_dicts: bool = False,   # noqa: A002
                            group_by_field: Optional[str] = None, group_size: int = 1, radius=None, range_filter=None, offset: int = 0):
        """Many sparse queries in CSR form (q_off int64 [nq + 1], q_terms uint32 term ids of the sparse index's vocabulary, q_vals
        float32; at most 64 strictly increasing terms per query) against the store's sparse index. Only rows that share a term
        with the query are hits. filter: a Milvus filter expression, or a list with one expression (or None) per query, through
        the mask cache. Returns (adjusted f64, raw f32, ids i64, levels i32), each [nq, top_k], in the order `search` returns
        hits; with as_dicts a list of `search`-shaped hit lists (`original_score` the sparse inner product). Bad arguments raise
        ValueError.
        group_by_field / group_size: as in `search` - the top_k best groups among the hits and the group_size best hit rows of
        each; the arrays are then [nq, top_k * group_size] and a fifth one follows, the hits' group values'
        ids; hit dicts carry the group value under metadata[group_by_field]. A filter stays a mask here (also a per-query list):
        the grouping is the whole store's.
        radius / range_filter / offset: as in `search`, on the sparse ranking - only hits with radius <
        score <= range_filter are ranked, the hits of ranks offset .. offset + top_k of that ranking are returned, then re-sorted
        by adjusted score. A bound is one number for every query or an array with one number per query. A row that shares no
        term with the query is no hit under any band. A bad bound, or one next to group_by_field, raises ValueError."""
        if group_by_field is not None:
            filter_expr.check_grouping(group_by_field, top_k, group_size)
        elif group_size != 1:
            raise ValueError("group_size needs group_by_field")
        if not self._int_in(top_k, 1, 128):
            raise ValueError(f"top_k={top_k!r}: an int in 1 .. 128")
        nq = len(np.asarray(q_off).reshape(-1)) - 1
        if nq < 0:
            raise ValueError("q_off holds nq + 1 offsets")
        radius, range_filter = range_search.check_bounds_per_query(radius, range_filter, nq)
        offset = range_search.check_offset(offset, top_k)
        banded = radius is not None or range_filter is not None or offset > 0
        if banded and group_by_field is not None:
            raise ValueError("radius / range_filter / offset cannot be combined with group_by_field")
        if isinstance(filter, (list, tuple)) and len(filter) != nq:
            raise ValueError(f"filter holds {len(filter)} expressions for {nq} queries")
        for e in (filter if isinstance(filter, (list, tuple)) else [filter]):
            if e is not None:
                filter_expr.compile(e)
        sp, _tx = self._sparse_index()
        index = self._index
        if int(top_k) > index.max_k:
            raise ValueError(f"top_k={top_k} exceeds the index's max_k={index.max_k} (ICD_GPU_MAX_K)")
        masks = None
        if filter is not None:
            masks = self._masks_for(index, filter, nq)
            if all(m is None for m in masks):
                masks = None
        q_terms, q_vals = np.asarray(q_terms, np.uint32).reshape(-1), np.asarray(q_vals, np.float32).reshape(-1)
        if group_by_field is not None:
            grouping, values = self._grouping(group_by_field, index, None, None)
            adj, raw, ids, levels, groups = self._sparse_lists(index, sp, q_off, q_terms, q_vals, int(top_k), masks, True, grouping, int(group_size))
            if not as_dicts:
                return adj, raw, ids, levels, groups
            return self._hit_lists(adj, raw, ids, (group_by_field, groups, values))
        if banded and nq > 0:
            band = range_search.SparseBandIndex(index, sp, masks)
            adj, raw, ids, levels = range_search.search_band(band, (np.asarray(q_off, np.int64).reshape(-1), q_terms, q_vals), int(top_k),
                                                             radius, range_filter, offset)
        else:
            adj, raw, ids, levels = self._sparse_lists(index, sp, q_off, q_terms, q_vals, int(top_k), masks, True)
        if not as_dicts:
            return adj, raw, ids, levels
        return self._hit_lists(adj, raw, ids)

    def search_text(self, text: str, top_k: int = 10, filter: Optional[str] = None,   # noqa: A002
                    group_by_field: Optional[str] = None, group_size: int = 1, radius: Optional[float] = None,
                    range_filter: Optional[float] = None, offset: int = 0,
                    search_params: Optional[Dict[str, Any]] = None) -> List[Dict[str, Any]]:
        """BM25 full-text search of ONE text over the sparse index's field: `search`-shaped hits, `original_score` the BM25 score,
        `score` the reweighted one. A text without a term of the vocabulary finds nothing. group_by_field / group_size: as in
        search_sparse_batch. radius / range_filter (also search_params={"params": {...}}) / offset: as in `search`, on the BM25
        score - a score floor, a ceiling to look under a crowd of titles that share a common term, a window deeper than 128.
        Bad arguments, or a bound next to group_by_field, raise ValueError."""
        if group_by_field is not None:
            filter_expr.check_grouping(group_by_field, top_k, group_size)
        elif group_size != 1:
            raise ValueError("group_size needs group_by_field")
        if not isinstance(text, str):
            raise ValueError("text: a string")
        self._one_filter(filter, "a list of filters needs a batch: search_sparse_batch")
        if not self._int_in(top_k, 1, 128):
            raise ValueError(f"top_k={top_k!r}: an int in 1 .. 128")
        radius, range_filter, offset, _banded = self._check_band(top_k, group_by_field, radius, range_filter, offset, search_params)
        _sp, tx = self._sparse_index()
        return self.search_sparse_batch(*tx.encode_queries([text]), top_k, filter=filter, as_dicts=True,
                                        group_by_field=group_by_field, group_size=group_size, radius=radius, range_filter=range_filter,
                                        offset=offset)[0]

    def search_text_iterator(self, text: str, batch_size: int = 10, limit: int = -1, filter: Optional[str] = None,   # noqa: A002
                             radius: Optional[float] = None, range_filter: Optional[float] = None,
                             search_params: Optional[Dict[str, Any]] = None) -> "range_search.SearchIterator":
        """search_iterator over the BM25 ranking of ONE text: next() returns the following batch_size hits
        of the text's hit ranking (inside the band, inside the filter's row mask) as a `search_text`-shaped list, [] when
        exhausted or after `limit` hits. Pages are disjoint and exact at any depth; batch_size <= 128. The iterator keeps the
        index, the sparse index, the mask and the store generation it started on: next() raises RuntimeError after the store
        changed. A text without a term of the vocabulary gives an exhausted iterator. Bad arguments raise ValueError."""
        radius, range_filter = range_search.check_bounds(radius, range_filter, search_params)
        if not isinstance(text, str):
            raise ValueError("text: a string")
        self._one_filter(filter, "search_text_iterator takes one filter expression")
        if filter is not None:
            filter_expr.compile(filter)
        band, query = None, None
        if self._live_index() is not None:
            sp, tx = self._sparse_index()
            index = self._index
            query = tx.encode_queries([text])
            mask = self._filter_mask(index, filter)
            if int(query[0][-1]) > 0 and (mask is None or mask.rows > 0):
                band = range_search.SparseBandIndex(index, sp, mask)
        client = self.client
        return range_search.SearchIterator(band, query, batch_size, limit, radius, range_filter, self._hits_to_dicts,
                                           lambda: (id(self.client), None if client is None else (client.generation, client.count)))

    def _hybrid_mixed(self, reqs, ranker, limit: int):
        """hybrid_search_batch with at least one sparse request: the dense requests as ONE search_batch-style sub-search, the
        sparse ones as ONE search_sparse_batch-style call, their raw lists interleaved into [nq, R, lmax] on the device, fused by
        fuse_lists. Returns device tensors."""
        index = self._ready_index()
        if index is None:
            raise RuntimeError(f"collection {self.collection_name} is empty or missing")
        sp, tx = self._sparse_index()
        dense = [r for r in reqs if r.anns_field == "vector"]
        sparse = [r for r in reqs if r.anns_field == "sparse"]
        sq = [hybrid.sparse_queries(r) for r in sparse]
        counts = {len(x) for x in sq}
        qd = None
        if dense:
            qd = hybrid.stack_requests(dense)
            counts.add(int(qd.shape[0]))
        if len(counts) != 1:
            raise ValueError("the requests' data must share one number of queries")
        nq, R = counts.pop(), len(reqs)
        lmax = max(r.limit for r in reqs)
        if lmax > index.max_k:
            raise ValueError(f"a request's limit exceeds the index's max_k={index.max_k} (ICD_GPU_MAX_K)")
        if nq * R > index.max_nq:
            raise ValueError(f"{nq} queries x {R} requests exceed the index's batch of {index.max_nq} (ICD_GPU_MAX_BATCH)")
        scores, ids, put = self._interleave_lists(index, reqs, nq, lmax)
        if dense:   # ONE banded / masked / plain sub-search over the nq * Rd vectors, as search_hybrid's step 1
            Rd, ld = len(dense), max(r.limit for r in dense)
            flat = qd.reshape(nq * Rd, -1) if hasattr(qd, "is_cuda") else np.ascontiguousarray(qd.reshape(nq * Rd, -1))
            per = [self._filter_mask(index, r.expr) for r in dense]
            lo = [r.radius for r in dense]
            hi = [r.range_filter for r in dense]
            if any(m is not None for m in per) or any(v is not None for v in lo + hi):
                bound = lambda vs, fill: None if all(v is None for v in vs) else np.tile(np.array([fill if v is None else v for v in vs], np.float32), nq)   # noqa: E731
                d_raw, d_ids, _lv = index.search_masked(flat, ld, per * nq, radius=bound(lo, -np.inf), range_filter=bound(hi, np.inf), reweighted=False)
            else:
                d_raw, d_ids = index.search(flat, ld)   # (AUTO: the same hits as EXACT, as search_hybrid's plain step 1)
            put("vector", d_raw, d_ids, ld)
        ls = max(r.limit for r in sparse)   # ONE sparse call over the nq * Rs queries (a caller sends at least one sparse request)
        csr = self._sparse_request_csr(tx, sq, nq)
        per = [self._filter_mask(index, r.expr) for r in sparse]
        s_raw, s_ids, _lv = self._sparse_lists(index, sp, *csr, ls, per * nq if any(m is not None for m in per) else None, False)
        put("sparse", s_raw, s_ids, ls)
        return index.fuse_lists(self._workspace_for("fusion", index, nq * R), scores, ids, [r.limit for r in reqs], limit, **self._ranker_kw(ranker)), nq, R

    @staticmethod
    def _ranker_kw(ranker):
        """search_hybrid's / fuse_lists' ranker keywords of an RRFRanker or a WeightedRanker"""
        return ({"ranker": "rrf", "rrf_c": ranker.k} if isinstance(ranker, hybrid.RRFRanker)
                else {"ranker": "weighted", "weights": ranker.weights, "norm": ranker.norm_score})

    @staticmethod
    def _sparse_request_csr(tx, sq, nq: int):
        """the nq * Rs sparse queries of a hybrid call as CSR, query-major: sq[r][q] is request r's text or {term id: weight} for query q"""
        return sparse_text.csr_from_pairs([tx.encode_query(x[q]) if isinstance(x[q], str) else sparse_text.query_from_dict(x[q], tx.vocab_size)
                                           for q in range(nq) for x in sq])

    @staticmethod
    def _interleave_lists(index, reqs, nq: int, width: int):
        """fuse_lists' input on the index's device: scores float32 (-inf) / ids int64 (-1) [nq, R, width], filled here, and
        put(field, scores, ids, w), which copies one side's raw lists ([nq * R_side, w], request order) into that side's columns"""
        import torch
        where = torch.device("cuda", index.device)
        scores = torch.full((nq, len(reqs), width), float("-inf"), dtype=torch.float32, device=where)
        ids = torch.full((nq, len(reqs), width), -1, dtype=torch.int64, device=where)

        def put(field, raw, lid, w):
            at = [i for i, r in enumerate(reqs) if r.anns_field == field]
            raw, lid = (torch.as_tensor(x).to(where).reshape(nq, len(at), w) for x in (raw, lid))
            for j, a in enumerate(at):
                scores[:, a, :w], ids[:, a, :w] = raw[:, j], lid[:, j]
        return scores, ids, put

    @staticmethod
    def _check_hybrid_grouping(reqs, limit, field, group_size):
        """the checks of a grouped hybrid search that need no store and no device (ValueError): the grouping arguments against the
        fused limit and every request's limit (groups times group_size fill at most 128 slots), no `param` band on any request, and
        ONE expression (or none) on all of them. Returns that expression."""
        filter_expr.check_grouping(field, limit, group_size)
        for i, r in enumerate(reqs):
            if r.radius is not None or r.range_filter is not None:
                raise ValueError(f"request {i}: radius / range_filter cannot be combined with group_by_field")
            if int(r.limit) * int(group_size) > filter_expr.MAX_GROUPED_HITS:
                raise ValueError(f"request {i}: limit * group_size = {int(r.limit) * int(group_size)} exceeds {filter_expr.MAX_GROUPED_HITS} hits "
                                 f"(limit={r.limit} groups of group_size={group_size})")
        keys = {None if r.expr is None else filter_expr.compile(r.expr) for r in reqs}
        if len(keys) != 1:
            raise ValueError("with group_by_field every request must carry the same expr (or none)")
        return reqs[0].expr

    def _hybrid_grouped(self, reqs, ranker, limit: int, field: str, group_size: int):
        """hybrid_search_batch with group_by_field. Dense requests only: search_hybrid with the grouping, on
        the expression's view with the view's grouping. With a sparse request: the dense side as ONE grouped search on the view,
        the sparse side as ONE grouped sparse search on the parent under the expression's mask, the raw lists interleaved on the
        device and fused on the parent with the parent's grouping. Returns ((adj, fused, ids, levels, bits, groups), nq, R, values)."""
        expr = self._check_hybrid_grouping(reqs, limit, field, group_size)
        s = int(group_size)
        index = self._ready_index()
        if index is None:
            raise RuntimeError(f"collection {self.collection_name} is empty or missing")
        dense = [r for r in reqs if r.anns_field == "vector"]
        sparse = [r for r in reqs if r.anns_field == "sparse"]
        R = len(reqs)
        qd = hybrid.stack_requests(dense) if dense else None
        sq = [hybrid.sparse_queries(r) for r in sparse]
        counts = {len(x) for x in sq} | ({int(qd.shape[0])} if dense else set())
        if len(counts) != 1:
            raise ValueError("the requests' data must share one number of queries")
        nq = counts.pop()
        target, rows, fkey = index, None, None
        if expr is not None:
            target, rows = self._filtered_index(expr)
            if target is not index:
                fkey = filter_expr.compile(expr)
        g_parent, values = self._grouping(field, index, None, None)
        if nq * R > min(index.max_nq, g_parent.max_nq):
            raise ValueError(f"{nq} queries x {R} requests exceed the grouped batch of {min(index.max_nq, g_parent.max_nq)}")
        if target is None:   # the expression selects no row: padding
            kk = limit * s
            return ((np.full((nq, kk), -np.inf), np.full((nq, kk), -np.inf), np.full((nq, kk), -1, np.int64), np.zeros((nq, kk), np.int32),
                     np.zeros((nq, kk), np.uint32), np.full((nq, kk), -1, np.int32)), nq, R, values)
        g_target = g_parent if target is index else self._grouping(field, target, rows, fkey)[0]
        if not sparse:
            out = target.search_hybrid(qd, [r.limit for r in reqs], limit, self._workspace_for("fusion", target, nq * R), grouping=g_target, group_size=s, **self._ranker_kw(ranker))
            return out, nq, R, values
        sp, tx = self._sparse_index()
        scores, ids, put = self._interleave_lists(index, reqs, nq, max(r.limit for r in reqs) * s)
        if dense:   # ONE grouped search over the nq * Rd vectors, on the view with the view's grouping (global ids come back)
            Rd, ld = len(dense), max(r.limit for r in dense)
            flat = qd.reshape(nq * Rd, -1) if hasattr(qd, "is_cuda") else np.ascontiguousarray(qd.reshape(nq * Rd, -1))
            d_raw, d_ids, _lv, _g = target.search_grouped(flat, ld, s, g_target, reweighted=False)
            put("vector", d_raw, d_ids, ld * s)
        Rs, ls = len(sparse), max(r.limit for r in sparse)   # ONE grouped sparse call over the nq * Rs queries, on the parent with the mask
        csr = self._sparse_request_csr(tx, sq, nq)
        mask = self._filter_mask(index, expr)
        s_raw, s_ids, _lv, _g = self._sparse_lists(index, sp, *csr, ls, None if mask is None else [mask] * (nq * Rs), False, g_parent, s)
        put("sparse", s_raw, s_ids, ls * s)
        out = index.fuse_lists(self._workspace_for("fusion", index, nq * R), scores, ids, [r.limit for r in reqs], limit, grouping=g_parent, group_size=s, **self._ranker_kw(ranker))
        return out, nq, R, values

    def hybrid_search_batch(self, reqs, ranker, limit: int = 10, as_dicts: bool = False, group_by_field: Optional[str] = None,
                            group_size: int = 1):
        """Milvus's hybrid_search for a batch: reqs is a list of 1 .. 8 hybrid_search.AnnSearchRequest whose data share one shape
        [nq, dim] (request r's vector of every query; numpy arrays, or torch CUDA tensors for device outputs); ranker an RRFRanker
        or WeightedRanker; limit the fused hits per query (1 .. 128). Every request's sub-list is exact, over its own expr's
        selection (through the mask cache; a selection of every row passes no mask) and its own param's radius / range_filter,
        and the lists are fused on the device. Returns (adjusted f64, fused f64, ids i64, levels i32, matched_requests bits), each
        [nq, limit], in the order `search` returns hits (adjusted = fused * level weight, one stable re-sort); with as_dicts a
        list of hybrid_search-shaped hit lists. Bad arguments raise ValueError before anything is loaded.
        group_by_field / group_size: Milvus's grouping on hybrid_search - every request's limit then counts
        GROUPS (limit * group_size <= 128), the sub-lists are grouped lists and the fused hits are grouped again: the `limit` best
        groups' group_size best rows, arrays [nq, limit * group_size] with a sixth one, the hits' group values' ids; hit dicts carry
        the group value under metadata[group_by_field]. Every request must then carry the same expr (or none) - the dense side runs
        on that expression's view with the view's grouping - and no `param` band; otherwise ValueError."""
        limit = hybrid.check_requests(reqs, ranker, limit)
        if group_by_field is not None:
            out, nq, R, values = self._hybrid_grouped(reqs, ranker, limit, group_by_field, group_size)
            return self._hybrid_dicts(out, nq, R, limit, (group_by_field, values)) if as_dicts else out
        if group_size != 1:
            raise ValueError("group_size needs group_by_field")
        if any(r.anns_field == "sparse" for r in reqs):   # (with dense requests only the path below is untouched)
            out, nq, R = self._hybrid_mixed(reqs, ranker, limit)
            return self._hybrid_dicts(out, nq, R, limit) if as_dicts else out
        q = hybrid.stack_requests(reqs)
        index = self._ready_index()
        if index is None:
            raise RuntimeError(f"collection {self.collection_name} is empty or missing")
        nq, R = int(q.shape[0]), len(reqs)
        if max(r.limit for r in reqs) > index.max_k:
            raise ValueError(f"a request's limit exceeds the index's max_k={index.max_k} (ICD_GPU_MAX_K)")
        if nq * R > index.max_nq:
            raise ValueError(f"{nq} queries x {R} requests exceed the index's batch of {index.max_nq} (ICD_GPU_MAX_BATCH)")
        per_req = [self._filter_mask(index, r.expr) for r in reqs]
        masks = [per_req] * nq if any(m is not None for m in per_req) else None
        lo = hi = None
        if any(r.radius is not None for r in reqs):
            lo = np.array([-np.inf if r.radius is None else r.radius for r in reqs], np.float32)
        if any(r.range_filter is not None for r in reqs):
            hi = np.array([np.inf if r.range_filter is None else r.range_filter for r in reqs], np.float32)
        out = index.search_hybrid(q, [r.limit for r in reqs], limit, self._workspace_for("fusion", index, nq * R), masks=masks, radius=lo,
                                  range_filter=hi, **self._ranker_kw(ranker))
        if not as_dicts:
            return out
        return self._hybrid_dicts(out, nq, R, limit)

    def _hybrid_dicts(self, out, nq: int, R: int, limit: int, group=None):
        """group: None, or (field, the field's sorted distinct values) of a grouped hybrid search (a sixth array holds the group ids)"""
        ids, bits = [t.cpu().numpy() if hasattr(t, "cpu") else t for t in (out[2], out[4])]
        res = []
        for qi, hits in enumerate(self._hit_lists(out[0], out[1], ids, None if group is None else (group[0], out[5], group[1]))):
            valid = [j for j in range(ids.shape[1]) if ids[qi][j] >= 0]
            for hit, j in zip(hits, valid):
                hit["fused_score"] = hit.pop("original_score")
                hit["matched_requests"] = [r for r in range(R) if (int(bits[qi][j]) >> r) & 1]
            res.append(hits)
        return res

    def hybrid_search(self, reqs, ranker, limit: int = 10, group_by_field: Optional[str] = None, group_size: int = 1) -> List[Dict[str, Any]]:
        """Milvus's hybrid_search for ONE query: every request's data is one vector. Returns a `search`-shaped hit list whose
        `score` is the reweighted fused score; `fused_score` (the ranker's value) and `matched_requests` (the indices of the
        requests whose list held the hit) replace `original_score`. group_by_field / group_size: as in hybrid_search_batch. Bad
        arguments raise ValueError."""
        limit = hybrid.check_requests(reqs, ranker, limit)
        if group_by_field is not None:
            self._check_hybrid_grouping(reqs, limit, group_by_field, group_size)
        elif group_size != 1:
            raise ValueError("group_size needs group_by_field")
        for r in reqs:
            if r.anns_field == "sparse":
                if isinstance(r.data, (list, tuple)) and len(r.data) != 1:
                    raise ValueError("hybrid_search takes one text per sparse request; hybrid_search_batch takes batches")
            elif np.ndim(r.data) > 2 or (np.ndim(r.data) == 2 and np.shape(r.data)[0] != 1):
                raise ValueError("hybrid_search takes one vector per request; hybrid_search_batch takes batches")
        return self.hybrid_search_batch(reqs, ranker, limit, as_dicts=True, group_by_field=group_by_field, group_size=group_size)[0]

    def _empty_hits(self, query_vectors, k: int, as_dicts: bool):
        nq = 1 if getattr(query_vectors, "ndim", 2) == 1 else int(query_vectors.shape[0])
        if as_dicts:
            return [[] for _ in range(nq)]
        if hasattr(query_vectors, "is_cuda") and query_vectors.is_cuda:
            import torch
            dev = query_vectors.device
            return (torch.full((nq, k), float("-inf"), dtype=torch.float64, device=dev),
                    torch.full((nq, k), float("-inf"), dtype=torch.float32, device=dev),
                    torch.full((nq, k), -1, dtype=torch.int64, device=dev), torch.zeros((nq, k), dtype=torch.int32, device=dev))
        return (np.full((nq, k), -np.inf, np.float64), np.full((nq, k), -np.inf, np.float32), np.full((nq, k), -1, np.int64),
                np.zeros((nq, k), np.int32))

    # ---- admin (same keys as the reference) -------------------------------------------------------------------------
    def get_collection_stats(self) -> Dict[str, Any]:
        try:
            exists = self.client is not None and self.client.exists()
            return {"collection_name": self.collection_name, "exists": exists, "dimension": self.dimension,
                    "num_entities": self.client.count if exists else 0}
        except Exception as exc:
            return {"error": str(exc)}

    def load_collection(self) -> bool:
        try:
            if self.client is None or not self.client.exists():
                logger.error("集合 %s 不存在", self.collection_name)
                return False
            self._load_collection_to_memory()
            return True
        except Exception as exc:
            logger.error("加载集合失败: %s", exc)
            return False

    def clear_collection(self) -> bool:
        try:
            self._drop_index()
            self.client.drop()
            self._setup_collection()
            return True
        except Exception as exc:
            logger.error("清空集合失败: %s", exc)
            return False

    def test_connection(self) -> Dict[str, Any]:
        mode = self.config.get("milvus", {}).get("mode", "local")
        try:
            if self.client is None:
                raise RuntimeError("客户端未连接")
            return {"connected": True, "mode": mode, "collection_stats": self.get_collection_stats(),
                    "client_type": "IcdIndex(MI355X)",
                    "local_info": {"db_path": self.config.get("milvus", {}).get("db_path")}}
        except Exception as exc:
            return {"connected": False, "error": str(exc), "mode": mode}

    def release_collection(self) -> Dict[str, Any]:
        try:
            if not self.client:
                return {"success": False, "message": "客户端未连接"}
            if not self.client.exists():
                return {"success": False, "message": f"集合 {self.collection_name} 不存在"}
            self._drop_index()
            return {"success": True, "message": f"集合 {self.collection_name} 内存已释放",
                    "collection_name": self.collection_name}
        except Exception as exc:
            return {"success": False, "message": f"释放集合内存失败: {exc}"}

    def get_collection_load_state(self) -> Dict[str, Any]:
        try:
            if not self.client:
                return {"loaded": False, "message": "客户端未连接"}
            if not self.client.exists():
                return {"loaded": False, "message": f"集合 {self.collection_name} 不存在"}
            loaded = bool(getattr(self, "_loaded", False)) and (self._index is not None or self.client.count == 0)
            return {"loaded": loaded, "state": "Loaded" if loaded else "NotLoad", "collection_name": self.collection_name}
        except Exception as exc:
            return {"loaded": False, "message": f"获取集合加载状态失败: {exc}"}

    def disconnect(self) -> Dict[str, Any]:
        try:
            if not self.client:
                return {"success": True, "message": "客户端已经断开"}
            release_result = self.release_collection()
            self._clear_views()
            self.client.close()
            self.client = None
            return {"success": True, "message": "Milvus连接已断开，资源已清理", "release_result": release_result}
        except Exception as exc:
            return {"success": False, "message": f"断开Milvus连接失败: {exc}"}

    def get_memory_usage(self) -> Dict[str, Any]:
        try:
            if not self.client:
                return {"memory_usage": 0, "message": "客户端未连接"}
            if not self.client.exists():
                return {"memory_usage": 0, "message": f"集合 {self.collection_name} 不存在"}
            stats = self.get_collection_stats()
            state = self.get_collection_load_state()
            out = {
                "collection_name": self.collection_name,
                "loaded": state.get("loaded", False),
                "load_state": state.get("state", "Unknown"),
                "num_entities": stats.get("num_entities", 0),
                "estimated_memory_mb": stats.get("num_entities", 0) * self.dimension * 4 / (1024 * 1024),
                "message": "内存使用为估算值（基于向量维度和实体数量）",
            }
            if self._index is not None:
                st = self._index.stats()
                out["hbm_bytes"] = st["bytes_corpus_f32"] + st["bytes_corpus_f16"] + st["bytes_workspace"]
            return out
        except Exception as exc:
            return {"memory_usage": 0, "message": f"获取内存使用情况失败: {exc}"}

    def health_check(self) -> Dict[str, Any]:
        try:
            conn = self.test_connection()
            state = self.get_collection_load_state()
            return {"healthy": conn.get("connected", False) and state.get("loaded", False), "connection": conn,
                    "load_state": state, "memory_usage": self.get_memory_usage(),
                    "timestamp": datetime.datetime.now().isoformat()}
        except Exception as exc:
            return {"healthy": False, "error": str(exc), "timestamp": datetime.datetime.now().isoformat()}

    def _calculate_level_weight(self, level: int) -> float:
        return {1: 1.2, 2: 1.0, 3: 0.8}.get(level, 1.0)
