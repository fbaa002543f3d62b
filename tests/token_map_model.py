"""RestrictTokenMap (restricts/allowlist.rs:184-244) restated in Python as a dict of lists: the model of the token-map
tests.  add_token appends; get_indices returns the list as inserted (duplicates and out-of-range indices kept);
create_allowlist sets bit i for every listed index below num_datapoints (RestrictAllowlist::add ignores the others)."""
import numpy as np


class TokenMapModel:
    def __init__(self, num_datapoints):
        self.num_datapoints = int(num_datapoints)
        self.token_to_indices = {}

    def add_token(self, index, token):
        self.token_to_indices.setdefault(int(token), []).append(int(index))

    def set_tokens(self, index, tokens):
        for t in tokens:
            self.add_token(index, t)

    def add_pairs(self, indices, tokens):
        """pair i is add_token(indices[i], tokens[i])"""
        for i, t in zip(np.asarray(indices).tolist(), np.asarray(tokens).tolist()):
            self.add_token(i, t)
        return self

    def get_indices(self, token):
        """the reference's Option<&[DatapointIndex]>: None for an unknown token, else insertion order"""
        return self.token_to_indices.get(int(token))

    def num_tokens(self):
        return len(self.token_to_indices)

    def stored_posting(self, token):
        """what the device map stores for a token: ascending, deduplicated, below num_datapoints"""
        ids = np.asarray(self.token_to_indices.get(int(token), []), np.int64)
        return np.unique(ids[ids < self.num_datapoints]).astype(np.uint32)

    def create_allowlist(self, tokens):
        """the words of create_allowlist(tokens)'s bitmap: ceil(num_datapoints / 64) uint64"""
        words = np.zeros(-(-self.num_datapoints // 64), np.uint64)
        for t in tokens:
            ids = self.stored_posting(t).astype(np.uint64)
            np.bitwise_or.at(words, (ids >> np.uint64(6)).astype(np.int64), np.uint64(1) << (ids & np.uint64(63)))
        return words

    def allow_bitmaps(self, token_lists, stride_words=None):
        """[nq, stride] block: row i = create_allowlist(token_lists[i]), gap words zero"""
        words = -(-self.num_datapoints // 64)
        stride = words if stride_words is None else int(stride_words)
        out = np.zeros((len(token_lists), stride), np.uint64)
        for i, tl in enumerate(token_lists):
            out[i, :words] = self.create_allowlist(tl)
        return out


def combine(op, a, b, bits):
    """numpy statement of the four block combinations over words [0, ceil(bits / 64)), the last word masked to bits;
    a / b: [nq, >= words] blocks or 1-D shared bitmaps.  op: 1 AND, 2 OR, 3 a & ~b, 4 ~a."""
    words = -(-bits // 64)
    a = np.asarray(a, np.uint64)[..., :words]
    if op != 4:
        b = np.asarray(b, np.uint64)[..., :words]
    r = {1: lambda: a & b, 2: lambda: a | b, 3: lambda: a & ~b, 4: lambda: ~a}[op]()
    r = np.array(np.broadcast_to(r, r.shape), np.uint64)
    if bits % 64 and words:
        r[..., words - 1] &= np.uint64((1 << (bits % 64)) - 1)
    return r
