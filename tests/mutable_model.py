"""Pure numpy model of the mutable index (include/scann_hip.h "mutable indexes"; mutator/mod.rs): the state machine of
MutableDataset over base + tombstones + delta, the rebuild counter of IncrementalUpdater, export / rebase, and the
expected search built on the CPU oracle.  Test infrastructure: the product never imports it.

The delta is modelled slot by slot (swap-remove included), so that the model can also say where a row sits -- the
searches must not depend on it."""
import numpy as np


class ModelError(Exception):
    code = 2


class InvalidArgument(ModelError):
    code = 3


class NotFound(ModelError):
    code = 5


class ResourceExhausted(ModelError):
    code = 8


class OutOfRange(ModelError):
    code = 11


EMPTY = 0xFFFFFFFF


class MutableModel:
    def __init__(self, base_rows, capacity, base_ids=None):
        self.capacity = int(capacity)
        self.next_index = 0
        self._set_base(base_rows, base_ids)

    def _set_base(self, base_rows, base_ids):
        self.base_rows = np.ascontiguousarray(base_rows, np.float32)
        n, self.dim = self.base_rows.shape
        self.base_ids = np.arange(n, dtype=np.int64) if base_ids is None else np.asarray(base_ids, np.int64)
        if self.base_ids.size != n or np.any(np.diff(self.base_ids) <= 0) or np.any(self.base_ids >= EMPTY):
            raise InvalidArgument("base_ids must be strictly ascending")
        self.identity = base_ids is None
        self.live = np.ones(n, bool)
        self.delta_ids = []          # slot -> id
        self.delta_rows = []         # slot -> row
        self.removed_delta = set()   # removed ids that have no base row
        self.pending_count = 0
        past = int(self.base_ids[-1]) + 1 if n else 0
        self.next_index = max(self.next_index, past)

    # ---- locations ----
    def base_row(self, id):
        j = int(np.searchsorted(self.base_ids, id))
        return j if j < self.base_ids.size and self.base_ids[j] == id else None

    def slot(self, id):
        return self.delta_ids.index(id) if id in self.delta_ids else None

    def known(self, id):
        return self.base_row(id) is not None or id in self.delta_ids or id in self.removed_delta

    def exists(self, id):
        if id in self.delta_ids:
            return True
        j = self.base_row(id)
        return j is not None and bool(self.live[j])

    def size(self):
        return int(self.live.sum()) + len(self.delta_ids)

    def pending(self):
        return self.pending_count

    def needs_rebuild(self, threshold):
        return self.pending_count >= threshold

    def get(self, id):
        if id in self.delta_ids:
            return self.delta_rows[self.delta_ids.index(id)].copy()
        j = self.base_row(id)
        if j is None or not self.live[j]:
            raise NotFound(id)
        return self.base_rows[j].copy()

    # ---- mutations: batches, applied in order, all or nothing ----
    @staticmethod
    def _rows(rows):
        r = np.asarray(rows, np.float32)
        return r[None] if r.ndim == 1 else r

    def add(self, rows):
        r = self._rows(rows)
        if r.shape[1] != self.dim:
            raise InvalidArgument("dim")
        if len(self.delta_ids) + r.shape[0] > self.capacity:
            raise ResourceExhausted("delta full")
        if self.next_index + r.shape[0] > EMPTY:
            raise OutOfRange("ids")
        ids = np.arange(self.next_index, self.next_index + r.shape[0], dtype=np.uint32)
        for id, row in zip(ids.tolist(), r):
            self.delta_ids.append(id)
            self.delta_rows.append(row.copy())
        self.next_index += r.shape[0]
        self.pending_count += r.shape[0]
        return int(ids[0]) if np.ndim(rows) == 1 else ids

    def remove(self, ids):
        ids = [int(i) for i in np.atleast_1d(ids)]
        for id in ids:
            if not self.known(id):
                raise NotFound(id)
        for id in ids:
            if id in self.delta_ids:      # swap-remove: the last row moves into the hole
                s = self.delta_ids.index(id)
                self.delta_ids[s] = self.delta_ids[-1]
                self.delta_rows[s] = self.delta_rows[-1]
                self.delta_ids.pop()
                self.delta_rows.pop()
                if self.base_row(id) is None:
                    self.removed_delta.add(id)
            else:
                j = self.base_row(id)
                if j is not None:
                    self.live[j] = False   # (already removed: absorbed)
            self.pending_count += 1

    def update(self, ids, rows):
        ids = [int(i) for i in np.atleast_1d(ids)]
        r = self._rows(rows)
        if r.shape[1] != self.dim or r.shape[0] != len(ids):   # (mod.rs:334-340: before the lookup)
            raise InvalidArgument("dim")
        for id in ids:
            if not self.known(id):
                raise NotFound(id)
        fresh = {id for id in ids if id not in self.delta_ids}
        if len(self.delta_ids) + len(fresh) > self.capacity:
            raise ResourceExhausted("delta full")
        for id, row in zip(ids, r):
            if id in self.delta_ids:
                self.delta_rows[self.delta_ids.index(id)] = row.copy()
            else:
                j = self.base_row(id)
                if j is not None:
                    self.live[j] = False
                self.removed_delta.discard(id)
                self.delta_ids.append(id)
                self.delta_rows.append(row.copy())
        self.pending_count += len(ids)

    # ---- export / rebase (compact) ----
    def export_live(self):
        """(rows, ids) of every live row, ascending by id"""
        ids = np.concatenate([self.base_ids[self.live], np.asarray(self.delta_ids, np.int64)])
        rows = np.concatenate([self.base_rows[self.live]] +
                              [np.asarray(self.delta_rows, np.float32).reshape(len(self.delta_rows), self.dim)])
        order = np.argsort(ids, kind="stable")
        return np.ascontiguousarray(rows[order]), ids[order].astype(np.uint32)

    def rebase(self, base_rows, base_ids=None):
        if np.asarray(base_rows).shape[1] != self.dim:
            raise InvalidArgument("dim")
        self._set_base(base_rows, base_ids)

    # ---- expected searches ----
    @staticmethod
    def allowed(ids, allow, allow_bits):
        """mask over external ids `ids` under the bitmap (words `allow`, capacity allow_bits); None = all"""
        ids = np.asarray(ids, np.uint64)
        if allow is None:
            return np.ones(ids.size, bool)
        allow = np.asarray(allow, np.uint64)
        cap = allow.size * 64 if allow_bits is None else int(allow_bits)
        ok = ids < np.uint64(cap)
        w = np.where(ok, ids >> np.uint64(6), np.uint64(0)).astype(np.int64)
        if allow.size == 0:
            return np.zeros(ids.size, bool)
        return ok & (((allow[np.minimum(w, allow.size - 1)] >> (ids & np.uint64(63))) & np.uint64(1)) == 1)

    def search_bf(self, measure, queries, k, allow=None, allow_bits=None):
        """brute-force base: the oracle's search over the live allowed rows in ascending id order, ids mapped back,
        each group of equal distances in ascending id order.  Returns per query (ids, dists)."""
        from oracle import pyoracle as orc
        rows, ids = self.export_live()
        ok = self.allowed(ids, allow, allow_bits)
        rows, ids = rows[ok], ids[ok]
        out = []
        if ids.size == 0 or k == 0:
            return [(np.zeros(0, np.uint32), np.zeros(0, np.float32)) for _ in queries]
        data, stride = orc.to_strided(rows)
        for q in np.asarray(queries, np.float32):
            oi, od = orc.bf_search(data, ids.size, self.dim, stride, measure, q, k)
            # TopK keeps the k smallest (distance, index) pairs, but drains equal distances in heap order
            # (top_k.rs:105-112 sorts by distance alone): the library's contract orders a tie by external id
            order = np.lexsort((ids[oi], od))
            out.append((ids[oi][order], od[order]))
        return out

    def base_allow_words(self, allow=None, allow_bits=None):
        """bitmap over BASE ROWS: live and allowed under the user's bitmap over external ids"""
        ok = self.live & self.allowed(self.base_ids, allow, allow_bits)
        words = np.zeros(max(1, -(-ok.size // 64)), np.uint64)
        j = np.flatnonzero(ok).astype(np.uint64)
        np.bitwise_or.at(words, (j >> np.uint64(6)).astype(np.int64), np.uint64(1) << (j & np.uint64(63)))
        return words, ok

    def merge_with_delta(self, base_lists, measure, queries, k, allow=None, allow_bits=None):
        """base_lists: per query (base ROW indices, dists) -- the base's filtered answer.  Adds the exact distances of
        the live allowed delta rows and keeps the k best by (distance, external id)."""
        from oracle import pyoracle as orc
        d_ids = np.asarray(self.delta_ids, np.int64)
        ok = self.allowed(d_ids, allow, allow_bits) if d_ids.size else np.zeros(0, bool)
        d_ids = d_ids[ok]
        out = []
        if d_ids.size:
            d_rows = np.asarray(self.delta_rows, np.float32).reshape(len(self.delta_rows), self.dim)[ok]
            data, stride = orc.to_strided(d_rows)
        for q, (bi, bd) in zip(np.asarray(queries, np.float32), base_lists):
            ids = self.base_ids[np.asarray(bi, np.int64)]
            dist = np.asarray(bd, np.float32)
            if d_ids.size:
                dd = orc.one_to_many(q, data, stride, d_ids.size, measure)
                ids = np.concatenate([ids, d_ids])
                dist = np.concatenate([dist, dd.astype(np.float32)])
            order = np.lexsort((ids, dist))[:k]
            out.append((ids[order].astype(np.uint32), dist[order]))
        return out

    def search_txh(self, oix, queries, k, allow=None, allow_bits=None, pre_reorder_k=0):
        """tree base: oix is the oracle's TxhIndex over the base rows; its filtered answer under live & user, merged
        with the delta.  pre_reorder_k = 0: from the index's multiplier."""
        from oracle import pyoracle as orc
        words, ok = self.base_allow_words(allow, allow_bits)
        keep_mult = oix.pre_reorder_multiplier
        lists = []
        try:
            oix.allow = None if ok.all() else words
            if pre_reorder_k:
                oix.pre_reorder_multiplier = float(pre_reorder_k) / float(k)
                assert orc.pre_reorder_k(k, oix.pre_reorder_multiplier) == pre_reorder_k
            for q in np.asarray(queries, np.float32):
                lists.append(orc.txh_search(oix, q, k))
        finally:
            oix.allow = None
            oix.pre_reorder_multiplier = keep_mult
        return self.merge_with_delta(lists, 0, queries, k, allow, allow_bits)

    def search_ah(self, codebook, codes, queries, k, pre_reorder_k, allow=None, allow_bits=None):
        """flat-hasher base: the AH oracle over the live allowed base rows (indices mapped back), merged with the delta"""
        from oracle import pyoracle as orc
        _, ok = self.base_allow_words(allow, allow_bits)
        rows = np.flatnonzero(ok)
        lists = []
        if rows.size:
            sub_codes = np.ascontiguousarray(np.asarray(codes)[rows])
            data, stride = orc.to_strided(self.base_rows[rows])
        for q in np.asarray(queries, np.float32):
            if rows.size == 0:
                lists.append((np.zeros(0, np.int64), np.zeros(0, np.float32)))
                continue
            oi, od = orc.ah_search_with_reordering(codebook, sub_codes, data, stride, q, k, pre_reorder_k)
            lists.append((rows[oi], od))
        return self.merge_with_delta(lists, 0, queries, k, allow, allow_bits)
