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
                      e.event_time.timestamp())
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
    [convergenceTol]."""

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
            tol=float(self.params.get("convergenceTol", 0.0)))
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
        """uint8 banned mask from white/black/category filters
        (ALSAlgorithm.scala:245-271 isCandidateItem). Device-resident:
        category membership comes from train-time masks, white/black
        lists are small index_put ops — nothing scans the catalog."""
        from predictionio_amd.templates.common import ids_tensor
        n = len(model.item_map)
        mask = None
        if q.white_list is not None:
            mask = torch.ones(n, dtype=torch.uint8, device=dev)
            mask[ids_tensor(q.white_list, model.item_map, dev)] = 0
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

    def predict(self, model: SimilarModel, query) -> PredictedResult:
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
        v, idx = topk_ops.topk_score(Xq, model.item_factors_norm, q.num,
                                     item_mask=mask)
        v, idx = v[0].cpu(), idx[0].cpu()
        return PredictedResult([
            ItemScore(model.item_inv[int(i)], float(s))
            for s, i in zip(v, idx) if i >= 0])

    def batch_predict(self, model: SimilarModel, queries):
        """Device-batched predict: ONE fused top-K launch over
        item_factors_norm for the whole batch. Per query, `categories`
        becomes a row of category bit words, and blackList + the query's
        own items a sorted ban list in one CSR. Queries with no known
        item give an empty result; queries with a whiteList (rare, and a
        batch-wide mask does not fit them) and models without category
        bits go through predict() one by one."""
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
        group = []  # (i, q, query item rows)
        for i, q in qs:
            if q.white_list is not None:
                out[i] = ALSAlgorithm.predict(self, model, q)
                continue
            rows = [model.item_map[x] for x in q.items
                    if x in model.item_map]
            if rows:
                group.append((i, q, rows))
            else:
                out[i] = PredictedResult([])
        if group:
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
            v, ix = topk_ops.topk_score(
                Xq, Yn, num, ban_indptr=ban_indptr, ban_indices=ban_indices,
                item_cats=bits.item_words, query_cats=query_cats)
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
        self.top_n = top_n          # item → [(other_item, count)]
        # the same lists as host numpy int32 [N, n]: id -1 / count 0 pad
        self.top_ids = top_ids
        self.top_cnt = top_cnt
        self.item_map = item_map
        self.items = items
        self.item_inv = item_map.inverse_array()


class CooccurrenceAlgorithm(Algorithm):
    """Params: n (top co-occurrences kept per item)
    (CooccurrenceAlgorithm.scala:49-108)."""

    def train(self, pd: PreparedData) -> CooccurrenceModel:
        """Pair counting as a per-item top-N over c[i][j] = number of
        users who viewed both (user-distinct) — replaces the reference's
        self-join + groupBy (CooccurrenceAlgorithm.scala:55-108). On a
        GPU the fused pair-count kernels (ops/cooccurrence.py) count each
        item row on chip and only the [N, n] result reaches the host; on
        CPU the same op runs its sparse A^T A reference."""
        from predictionio_amd.ops.cooccurrence import cooccurrence_topn
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
        u = torch.tensor([user_map[v.user] for v in pd.view_events],
                         dtype=torch.int64, device=device)
        i = torch.tensor([item_map[v.item] for v in pd.view_events],
                         dtype=torch.int64, device=device)
        # user-distinct (view twice ≠ two pairs): the op dedups the pairs
        ids, cnt = cooccurrence_topn(u, i, n_users, n_items, n_keep)
        top_ids, top_cnt = ids.cpu().numpy(), cnt.cpu().numpy()
        top_n: Dict[int, List[Tuple[int, int]]] = {}
        for it in (top_ids[:, 0] >= 0).nonzero()[0].tolist():
            k = int((top_ids[it] >= 0).sum())
            top_n[it] = list(zip(top_ids[it, :k].tolist(),
                                 top_cnt[it, :k].tolist()))
        return CooccurrenceModel(top_n, item_map, pd.items,
                                 top_ids=top_ids, top_cnt=top_cnt)

    def predict(self, model: CooccurrenceModel, query) -> PredictedResult:
        q = query if isinstance(query, Query) else Query.from_json(query)
        counts: Dict[int, int] = defaultdict(int)
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
                      e.event_time.timestamp())
            for e in event_store.find(app, entity_type="user",
                                      event_names=["follow"],
                                      target_entity_type="user")
        ]
        return TrainingData({}, {}, follows)


class RecommendedUserAlgorithm(ALSAlgorithm):
    """Trains implicit ALS on follow events; the 'item' side is the
    followed users, so predict returns similar USERS
    (recommended-user ALSAlgorithm.scala)."""

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
