"""Similar-Product engine template (MI355X-native).

Parity with examples/scala-parallel-similarproduct/recommended-user →
actually the base template (examples/scala-parallel-similarproduct/*):
- Query {items, num, [categories], [whiteList], [blackList]}
  (src/main/scala/Engine.scala)
- DataSource aggregates $set user/item properties + view events
  (DataSource.scala:133 total)
- ALSAlgorithm (P2L): implicit-style ALS on view events with latest-wins
  (user, item) dedup (ALSAlgorithm.scala:88-120), productFeatures collected
  local (:130-143); predict = sum of cosine similarities of the query
  items' factors vs ALL item factors, filtered by white/black/category,
  top-num (:168-271 — the reference's .par loop + hand-rolled cosine +
  bounded PriorityQueue)
- CooccurrenceAlgorithm: user-distinct item pairs → pair counts → top-N
  co-occurring items (CooccurrenceAlgorithm.scala:49-108)

MI355X design: cosine scoring = L2-normalize factors once at train time,
then the summed-query-vector dot against all items in one fused masked
top-K kernel launch.
"""

from __future__ import annotations

from collections import defaultdict
from dataclasses import dataclass
from typing import Any, Dict, List, Optional, Set, Tuple

import torch

from predictionio_amd.parallel import dist as pdist

from predictionio_amd.controller import (
    Algorithm, DataSource as BaseDataSource, Engine, EngineFactory,
    Preparator as BasePreparator, SanityCheck, Serving as BaseServing,
)
from predictionio_amd.data import event_store
from predictionio_amd.data.bimap import BiMap
from predictionio_amd.models.als import ALSParams, train_als
from predictionio_amd.ops import topk as topk_ops


@dataclass
class Item:
    categories: Optional[List[str]]


@dataclass
class ViewEvent:
    user: str
    item: str
    t: float
    name: str = "view"   # the event's name (DataSource eventNames)


@dataclass
class TrainingData(SanityCheck):
    users: Dict[str, dict]
    items: Dict[str, Item]
    view_events: List[ViewEvent]

    def sanity_check(self):
        if not self.view_events:
            raise ValueError("view events are empty")


@dataclass
class PreparedData:
    users: Dict[str, dict]
    items: Dict[str, Item]
    view_events: List[ViewEvent]


@dataclass
class Query:
    items: List[str]
    num: int
    categories: Optional[List[str]] = None
    white_list: Optional[List[str]] = None
    black_list: Optional[List[str]] = None

    @staticmethod
    def from_json(d: Dict[str, Any]) -> "Query":
        return Query(items=list(d["items"]), num=int(d.get("num", 10)),
                     categories=d.get("categories"),
                     white_list=d.get("whiteList"),
                     black_list=d.get("blackList"))


@dataclass
class ItemScore:
    item: str
    score: float


@dataclass
class PredictedResult:
    item_scores: List[ItemScore]

    def to_json(self):
        return {"itemScores": [{"item": s.item, "score": s.score}
                               for s in self.item_scores]}


class DataSource(BaseDataSource):
    """Params: appName."""

    def read_training(self) -> TrainingData:
        """Params: appName, [eventNames] — the train-with-rate-event
        variant passes ["rate"] (or mixes) and the events still feed the
        implicit trainer as unit preferences."""
        app = self.params["appName"]
        names = list(self.params.get("eventNames", ["view"]))
        users = {eid: pm.to_dict() for eid, pm in
                 event_store.aggregate_properties(app, "user").items()}
        items = {eid: Item(categories=pm.get_opt("categories"))
                 for eid, pm in
                 event_store.aggregate_properties(app, "item").items()}
        views = [
            ViewEvent(e.entity_id, e.target_entity_id,
                      e.event_time.timestamp(), e.event)
            for e in event_store.find(app, entity_type="user",
                                      event_names=names,
                                      target_entity_type="item")
        ]
        return TrainingData(users, items, views)


class Preparator(BasePreparator):
    def prepare(self, td: TrainingData) -> PreparedData:
        return PreparedData(td.users, td.items, td.view_events)


class SimilarModel:
    """Normalized item factors + maps + categories (P2L local model)."""

    def __init__(self, item_factors_norm: torch.Tensor, item_map: BiMap,
                 items: Dict[str, Item], category_masks=None,
                 category_bits=None, category_bits_built: bool = False):
        """category_bits_built=True says `category_bits` is the outcome
        of CategoryBits.build, so None means "too many categories";
        otherwise a missing value is built on first use."""
        self.item_factors_norm = item_factors_norm  # L2-normalized rows
        self.item_map = item_map
        self.items = items
        self.item_inv = item_map.inverse_array()
        self.category_masks = category_masks
        self.category_bits = category_bits
        self._cat_bits_built = (category_bits_built
                                or category_bits is not None)

    def cat_bits(self):
        """Category bit words for the fused per-query filter (train-time;
        lazily rebuilt for models persisted before they existed). None
        when the catalog has too many categories for the bit words."""
        if not getattr(self, "_cat_bits_built", False):
            from predictionio_amd.templates.common import CategoryBits
            self.category_bits = CategoryBits.build(
                self.items, self.item_map, self.item_factors_norm.device)
            self._cat_bits_built = True
        return self.category_bits

    def item_inv_np(self):
        """item index -> external id as a numpy array (vectorized
        fancy-indexing for the batch-predict epilogue)."""
        if getattr(self, "_item_inv_np", None) is None:
            import numpy as np
            self._item_inv_np = np.asarray(self.item_inv, dtype=object)
        return self._item_inv_np

    def cat_masks(self):
        """Device category masks (built at train time; lazily rebuilt
        for models persisted before round 2)."""
        if self.category_masks is None:
            from predictionio_amd.templates.common import CategoryMasks
            self.category_masks = CategoryMasks.build(
                self.items, self.item_map, self.item_factors_norm.device)
        return self.category_masks


class ALSAlgorithm(Algorithm):
    """Params: rank, numIterations, lambda, alpha, [seed], [lossEvery],
    [convergenceTol].
    [nonnegative]: factors constrained to >= 0 (MLlib's setNonnegative)."""

    def train(self, pd: PreparedData) -> SimilarModel:
        if not pd.view_events:
            raise ValueError("no view events")
        user_map = BiMap.string_int(v.user for v in pd.view_events)
        # include property-only items so queries on them resolve
        item_keys = [v.item for v in pd.view_events] + list(pd.items)
        item_map = BiMap.string_int(item_keys)
        # latest-wins dedup on (user, item) (ALSAlgorithm.scala:88-120):
        # sort by time then aggregate 'latest'; implicit weight 1 per view
        evs = sorted(pd.view_events, key=lambda v: v.t)
        users = torch.tensor([user_map[v.user] for v in evs],
                             dtype=torch.int32)
        items = torch.tensor([item_map[v.item] for v in evs],
                             dtype=torch.int32)
        vals = torch.ones(len(evs))
        from predictionio_amd.ops import als as als_ops
        users, items, vals = als_ops.aggregate_ratings(
            users, items, vals, len(item_map), "sum")
        p = ALSParams(
            rank=int(self.params.get("rank", 10)),
            iterations=int(self.params.get("numIterations", 20)),
            lambda_=float(self.params.get("lambda", 0.01)),
            alpha=float(self.params.get("alpha", 1.0)),
            implicit=True, seed=self.params.get("seed"),
            loss_every=int(self.params.get("lossEvery", 0)),
            tol=float(self.params.get("convergenceTol", 0.0)),
            nonnegative=bool(self.params.get("nonnegative", False)))
        device = pdist.compute_device()
        _, Y = train_als(users, items, vals, len(user_map), len(item_map),
                         p, device=device)
        Yn = torch.nn.functional.normalize(Y, dim=1, eps=1e-9)
        from predictionio_amd.templates.common import (
            CategoryBits, CategoryMasks,
        )
        cm = CategoryMasks.build(pd.items, item_map, Yn.device)
        cb = CategoryBits.build(pd.items, item_map, Yn.device)
        return SimilarModel(Yn, item_map, pd.items, cm, cb,
                            category_bits_built=True)

    def _masks(self, model: SimilarModel, q: Query,
               dev) -> Optional[torch.Tensor]:
        """uint8 banned mask from black/category filters
        (ALSAlgorithm.scala:245-271 isCandidateItem). Device-resident:
        category membership comes from train-time masks, the blackList
        is a small index_put op — nothing scans the catalog. A whiteList
        is not part of the mask: it goes to the kernel as the query's
        candidate list (_cands)."""
        from predictionio_amd.templates.common import ids_tensor
        n = len(model.item_map)
        mask = None
        if q.categories is not None:
            cm = model.cat_masks().banned_outside(q.categories).to(dev)
            mask = cm if mask is None else (mask | cm)
        if q.black_list:
            if mask is None:
                mask = torch.zeros(n, dtype=torch.uint8, device=dev)
            mask[ids_tensor(q.black_list, model.item_map, dev)] = 1
        # query items themselves are never returned (reference excludes them)
        if mask is None:
            mask = torch.zeros(n, dtype=torch.uint8, device=dev)
        mask[ids_tensor(q.items, model.item_map, dev)] = 1
        return mask

    # batch_predict keeps whiteList queries in the batch (one candidate-
    # list launch); False sends each through predict(), which passes its
    # own one-row candidate list
    batch_white_lists = True

    @staticmethod
    def _cands(model, q: Query) -> List[int]:
        """The whiteList as a sorted candidate list of item rows."""
        return sorted({model.item_map[x] for x in q.white_list
                       if x in model.item_map})

    def predict(self, model: SimilarModel, query) -> PredictedResult:
        from predictionio_amd.templates.common import ban_csr
        q = query if isinstance(query, Query) else Query.from_json(query)
        rows = [model.item_map[i] for i in q.items
                if i in model.item_map]
        if not rows:
            return PredictedResult([])
        dev = model.item_factors_norm.device
        # sum of cosines = (sum of normalized query vectors) . Yn
        Xq = model.item_factors_norm[torch.tensor(rows, device=dev)] \
            .sum(dim=0, keepdim=True)
        mask = self._masks(model, q, dev)
        kw = {}
        if q.white_list is not None:
            kw["cand_indptr"], kw["cand_indices"] = ban_csr(
                [self._cands(model, q)], dev)
        v, idx = topk_ops.topk_score(Xq, model.item_factors_norm, q.num,
                                     item_mask=mask, **kw)
        v, idx = v[0].cpu(), idx[0].cpu()
        return PredictedResult([
            ItemScore(model.item_inv[int(i)], float(s))
            for s, i in zip(v, idx) if i >= 0])

    def batch_predict(self, model: SimilarModel, queries):
        """Device-batched predict: ONE fused top-K launch over
        item_factors_norm for the batch's plain queries and one
        candidate-list launch for its whiteList queries. Per query,
        `categories` becomes a row of category bit words, blackList +
        the query's own items a sorted ban list in one CSR, and a
        whiteList a row of the candidate CSR. Queries with no known item
        give an empty result; models without category bits go through
        predict() one by one."""
        import numpy as np
        from predictionio_amd.templates.common import ban_csr
        qs = [(i, q if isinstance(q, Query) else Query.from_json(q))
              for i, q in queries]
        bits = model.cat_bits()
        # the per-query fallback is THIS class's predict on the parsed
        # Query — a subclass (RecommendedUserAlgorithm) overrides predict
        # for its own query type and hands batch_predict ready Queries
        if bits is None:
            return [(i, ALSAlgorithm.predict(self, model, q))
                    for i, q in qs]
        out: Dict[int, PredictedResult] = {}
        groups = ([], [])  # (i, q, query item rows): plain, whiteList
        for i, q in qs:
            if q.white_list is not None and not self.batch_white_lists:
                out[i] = ALSAlgorithm.predict(self, model, q)
                continue
            rows = [model.item_map[x] for x in q.items
                    if x in model.item_map]
            if rows:
                groups[q.white_list is not None].append((i, q, rows))
            else:
                out[i] = PredictedResult([])
        for white, group in enumerate(groups):
            if not group:
                continue
            Yn = model.item_factors_norm
            dev = Yn.device
            # sum of cosines = (sum of normalized query vectors) . Yn
            rows = torch.tensor([r for g in group for r in g[2]],
                                device=dev)
            seg = torch.tensor(
                [k for k, g in enumerate(group) for _ in g[2]], device=dev)
            Xq = torch.zeros((len(group), Yn.shape[1]), dtype=Yn.dtype,
                             device=dev).index_add_(0, seg, Yn[rows])
            # the query's own items are never returned
            ban_indptr, ban_indices = ban_csr(
                [sorted(set(g[2]) | {model.item_map[x]
                                     for x in (g[1].black_list or [])
                                     if x in model.item_map})
                 for g in group], dev)
            query_cats = torch.from_numpy(np.stack(
                [bits.query_words(g[1].categories) for g in group])).to(dev)
            num = max(g[1].num for g in group)
            kw = {}
            if white:
                kw["cand_indptr"], kw["cand_indices"] = ban_csr(
                    [self._cands(model, g[1]) for g in group], dev)
            v, ix = topk_ops.topk_score(
                Xq, Yn, num, ban_indptr=ban_indptr, ban_indices=ban_indices,
                item_cats=bits.item_words, query_cats=query_cats, **kw)
            v_np = v.cpu().numpy()
            ix_np = ix.cpu().numpy()
            names = model.item_inv_np()[np.clip(ix_np, 0, None)]
            for r, (i, q, _) in enumerate(group):
                out[i] = PredictedResult(
                    [ItemScore(nm, float(s)) for nm, s, it in
                     zip(names[r, :q.num], v_np[r, :q.num],
                         ix_np[r, :q.num]) if it >= 0])
        return [(i, out[i]) for i, _ in qs]


class CooccurrenceModel:
    def __init__(self, top_n: Dict[int, List[Tuple[int, int]]],
                 item_map: BiMap, items: Dict[str, Item],
                 top_ids=None, top_cnt=None):
        self.top_n = top_n          # item → [(other_item, count or score)]
        # the same lists as host numpy [N, n]: id -1 / count 0 pad; int32,
        # the scores of scoring="llr" float32
        self.top_ids = top_ids
        self.top_cnt = top_cnt
        self.item_map = item_map
        self.items = items
        self.item_inv = item_map.inverse_array()

    def device_table(self):
        """(top_ids, top_scores) as tensors on the serving device, built
        from the host copies and checked against indicator_topk's table
        contract once, on first use; None for a model without a table."""
        if self.top_ids is None:
            return None
        if getattr(self, "_device_table", None) is None:
            from predictionio_amd.ops.cooccurrence import (
                check_indicator_table,
            )
            dev = getattr(self, "_device", None) or (
                torch.device("cuda") if torch.cuda.is_available()
                else torch.device("cpu"))
            ids = torch.from_numpy(self.top_ids).to(dev).contiguous()
            sc = torch.from_numpy(self.top_cnt).to(dev).contiguous()
            check_indicator_table(ids, sc, len(self.item_map))
            self._device_table = (ids, sc)
        return self._device_table

    def to(self, device) -> "CooccurrenceModel":
        """Serve from `device`: the table and the category words are
        rebuilt there on their next use."""
        self._device = torch.device(device)
        self._device_table = None
        self._cat_bits_built = False
        return self

    def cat_bits(self):
        """CategoryBits words on the table's device, built on first use;
        None when the catalog has more than 127 categories."""
        if not getattr(self, "_cat_bits_built", False):
            from predictionio_amd.templates.common import CategoryBits
            self.category_bits = CategoryBits.build(
                self.items, self.item_map, self.device_table()[0].device)
            self._cat_bits_built = True
        return self.category_bits


class CooccurrenceAlgorithm(Algorithm):
    """Params: n (top co-occurrences kept per item)
    (CooccurrenceAlgorithm.scala:49-108); scoring, "count" (default) or
    "llr" (log-likelihood ratio: a merely popular item scores near 0);
    targetEvent, unset by default: when set, rows are counted over the
    events named `event` (default: all read events), columns over the
    targetEvent events ("viewed this, bought ..."), the item itself
    excluded."""

    def train(self, pd: PreparedData) -> CooccurrenceModel:
        """Pair counting as a per-item top-N over c[i][j] = number of
        users who viewed both (user-distinct) — replaces the reference's
        self-join + groupBy (CooccurrenceAlgorithm.scala:55-108). On a
        GPU the fused pair-count kernels (ops/cooccurrence.py) count each
        item row on chip and only the [N, n] result reaches the host; on
        CPU the same op runs its sparse A^T A reference."""
        from predictionio_amd.ops.cooccurrence import (
            cooccurrence_topn, cross_occurrence_topn,
        )
        scoring = self.params.get("scoring", "count")
        target = self.params.get("targetEvent")
        item_map = BiMap.string_int(
            [v.item for v in pd.view_events] + list(pd.items))
        user_map = BiMap.string_int(v.user for v in pd.view_events)
        n_keep = int(self.params.get("n", 10))
        n_items = len(item_map)
        n_users = len(user_map)
        if not pd.view_events:
            return CooccurrenceModel({}, item_map, pd.items)
        device = (torch.device("cuda") if torch.cuda.is_available()
                  else torch.device("cpu"))

        def pairs(events):
            return (torch.tensor([user_map[v.user] for v in events],
                                 dtype=torch.int64, device=device),
                    torch.tensor([item_map[v.item] for v in events],
                                 dtype=torch.int64, device=device))

        # user-distinct (view twice ≠ two pairs): the op dedups the pairs
        if target is None:
            u, i = pairs(pd.view_events)
            ids, cnt = cooccurrence_topn(u, i, n_users, n_items, n_keep,
                                         score=scoring)
        else:
            source = self.params.get("event")
            ua, ia = pairs([v for v in pd.view_events
                            if source is None or v.name == source])
            ub, ib = pairs([v for v in pd.view_events if v.name == target])
            ids, cnt = cross_occurrence_topn(
                ua, ia, n_items, ub, ib, n_items, n_users, n_keep,
                score=scoring, exclude_self=True)
        top_ids, top_cnt = ids.cpu().numpy(), cnt.cpu().numpy()
        top_n: Dict[int, List[Tuple[int, int]]] = {}
        for it in (top_ids[:, 0] >= 0).nonzero()[0].tolist():
            k = int((top_ids[it] >= 0).sum())
            top_n[it] = list(zip(top_ids[it, :k].tolist(),
                                 top_cnt[it, :k].tolist()))
        model = CooccurrenceModel(top_n, item_map, pd.items,
                                  top_ids=top_ids, top_cnt=top_cnt)
        model.device_table()  # built and checked once, for batch_predict
        model.cat_bits()
        return model

    def predict(self, model: CooccurrenceModel, query) -> PredictedResult:
        q = query if isinstance(query, Query) else Query.from_json(query)
        counts: Dict[int, float] = defaultdict(int)  # or summed scores
        qidx = {model.item_map.get(i) for i in q.items}
        for i in q.items:
            ii = model.item_map.get(i)
            if ii is None:
                continue
            for other, c in model.top_n.get(ii, []):
                counts[other] += c
        white = ({model.item_map.get(i) for i in q.white_list}
                 if q.white_list is not None else None)
        black = {model.item_map.get(i) for i in (q.black_list or [])}
        cats = set(q.categories) if q.categories is not None else None

        def ok(i: int) -> bool:
            if i in qidx or i in black:
                return False
            if white is not None and i not in white:
                return False
            if cats is not None:
                meta = model.items.get(model.item_inv[i])
                if not (meta and meta.categories
                        and cats & set(meta.categories)):
                    return False
            return True

        ranked = sorted(((c, i) for i, c in counts.items() if ok(i)),
                        reverse=True)[:q.num]
        return PredictedResult([
            ItemScore(model.item_inv[i], float(c)) for c, i in ranked])

    def batch_predict(self, model: CooccurrenceModel, queries):
        """Device-batched predict: one indicator_topk call (two when some
        queries carry a whiteList: they form a group of their own, so the
        others are not restricted by an allow list). Per query the known
        items become a row of the query CSR, blackList a row of the ban
        CSR, whiteList a row of the allow CSR and `categories` a row of
        category bit words; the query's own items are excluded by the op.
        Unknown items are dropped, as in predict. Scores of an "llr"
        model are the canonical fp32 sums of the op where predict adds in
        double. One documented difference: on equal scores the order here
        is item index ascending, in predict descending. Queries predict
        treats specially (a repeated item, num outside [1, 1024]), models
        without a table and catalogs with more than 127 categories go
        through predict one by one."""
        import numpy as np
        from predictionio_amd.ops.cooccurrence import (
            IND_K_MAX, indicator_topk,
        )
        from predictionio_amd.templates.common import ban_csr
        qs = [(i, q if isinstance(q, Query) else Query.from_json(q))
              for i, q in queries]
        table = model.device_table()
        bits = model.cat_bits() if table is not None else None
        if bits is None:
            return [(i, self.predict(model, q)) for i, q in qs]
        ids_t, sc_t = table
        dev = ids_t.device
        imap = model.item_map

        def known(names):
            return sorted({imap[x] for x in names if x in imap})

        out: Dict[int, PredictedResult] = {}
        groups = ([], [])  # (i, q, query item rows): plain, whiteList
        for i, q in qs:
            rows = known(q.items)
            if (len(rows) != sum(x in imap for x in q.items)
                    or not 1 <= q.num <= IND_K_MAX):
                out[i] = self.predict(model, q)
            elif rows:
                groups[q.white_list is not None].append((i, q, rows))
            else:
                out[i] = PredictedResult([])
        inv = np.asarray(model.item_inv, dtype=object)
        for white, group in enumerate(groups):
            if not group:
                continue
            q_indptr, q_items = ban_csr([g[2] for g in group], dev)
            ban_indptr, ban_indices = ban_csr(
                [known(g[1].black_list or []) for g in group], dev)
            kw = {}
            if white:
                kw["allow_indptr"], kw["allow_indices"] = ban_csr(
                    [known(g[1].white_list) for g in group], dev)
            query_cats = torch.from_numpy(np.stack(
                [bits.query_words(g[1].categories) for g in group])).to(dev)
            ids, sc = indicator_topk(
                ids_t, sc_t, q_indptr, q_items, max(g[1].num for g in group),
                n_cols=len(imap), ban_indptr=ban_indptr,
                ban_indices=ban_indices, item_cats=bits.item_words,
                query_cats=query_cats, exclude_query=True, check_table=False,
                **kw)
            ids_np, sc_np = ids.cpu().numpy(), sc.cpu().numpy()
            names = inv[np.clip(ids_np, 0, None)]
            for r, (i, q, _) in enumerate(group):
                out[i] = PredictedResult(
                    [ItemScore(nm, float(s)) for nm, s, it in
                     zip(names[r, :q.num], sc_np[r, :q.num],
                         ids_np[r, :q.num]) if it >= 0])
        return [(i, out[i]) for i, _ in qs]


class Serving(BaseServing):
    def serve(self, query, predictions) -> PredictedResult:
        return predictions[0]


class SimilarProductEngine(EngineFactory):
    @classmethod
    def apply(cls) -> Engine:
        return Engine(
            data_source_class=DataSource,
            preparator_class=Preparator,
            algorithm_class={"als": ALSAlgorithm,
                             "cooccurrence": CooccurrenceAlgorithm,
                             "": ALSAlgorithm},
            serving_class=Serving)


# --------------------------------------------------------------------------
# recommended-user variant (examples/scala-parallel-similarproduct/
# recommended-user): the same cosine-kNN machinery over USER factors —
# "users who follow the query users also follow these users". Events are
# `follow` (user → similarUser); the model keeps the followed-user factors.
# --------------------------------------------------------------------------


@dataclass
class UserQuery:
    users: List[str]
    num: int
    white_list: Optional[List[str]] = None
    black_list: Optional[List[str]] = None

    @staticmethod
    def from_json(d: Dict[str, Any]) -> "UserQuery":
        return UserQuery(users=list(d["users"]), num=int(d.get("num", 10)),
                         white_list=d.get("whiteList"),
                         black_list=d.get("blackList"))


class FollowDataSource(BaseDataSource):
    """Reads `follow` events (user → similarUser entity type `user`)."""

    def read_training(self) -> TrainingData:
        app = self.params["appName"]
        follows = [
            ViewEvent(e.entity_id, e.target_entity_id,
                      e.event_time.timestamp(), e.event)
            for e in event_store.find(app, entity_type="user",
                                      event_names=["follow"],
                                      target_entity_type="user")
        ]
        return TrainingData({}, {}, follows)


class RecommendedUserAlgorithm(ALSAlgorithm):
    """Trains implicit ALS on follow events; the 'item' side is the
    followed users, so predict returns similar USERS
    (recommended-user ALSAlgorithm.scala). Its whiteList queries keep
    the per-query route of batch_predict (each a one-row candidate-list
    call)."""

    batch_white_lists = False

    def predict(self, model: SimilarModel, query) -> PredictedResult:
        q = query if isinstance(query, UserQuery) \
            else UserQuery.from_json(query)
        return super().predict(
            model, Query(items=q.users, num=q.num,
                         white_list=q.white_list, black_list=q.black_list))

    def batch_predict(self, model: SimilarModel, queries):
        return super().batch_predict(
            model,
            [(i, Query(items=q.users, num=q.num, white_list=q.white_list,
                       black_list=q.black_list))
             for i, q in ((i, q if isinstance(q, UserQuery)
                           else UserQuery.from_json(q))
                          for i, q in queries)])


class RecommendedUserEngine(EngineFactory):
    @classmethod
    def apply(cls) -> Engine:
        return Engine(
            data_source_class=FollowDataSource,
            preparator_class=Preparator,
            algorithm_class={"als": RecommendedUserAlgorithm,
                             "": RecommendedUserAlgorithm},
            serving_class=Serving)
