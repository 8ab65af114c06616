"""Host model of the exact-key f-gram index, in plain Python integers, and the hostile index states built with it.

The first part restates the `__host__ __device__` functions of scone_amd/csrc/scone_common.h that decide where a key goes
(`scone_pack_key` in both layouts, `scone_hash_key`, `scone_bucket_home`, `scone_bucket_step`, `scone_bloom_bit`) and the bitmap
size rule of `scone_create`.  tests/test_index_model_host.py holds every one of them to the product's own functions through
tests/index_model_check.cpp.  Nothing here is read by the product, and nothing here reads the product.

The model never says which SLOT a key lands in: insertion is concurrent and the slot depends on the order.  It derives only what
holds for every order -- how many keys are homed in each bucket, which bitmap bits are set, which (lo, ext) a window packs to.

The second part are the generators.  Each is seeded and deterministic and returns
`(keys [n, max_n] uint32, lens [n] uint8, index_capacity, batch, facts)`; `batch` is a `Batch` (the same windows laid out as a
rectangle [B, T] and as a packed stream with ragged `cu_seqlens`, one empty sequence included, both with -1 tokens), `facts` the
counts that prove the state is what its name says (every key of the index occurs in the batch as a window, in both forms) -- computed from the arrays that are returned, never from what the generator
meant to build."""

import collections

import numpy as np

M64 = (1 << 64) - 1
M32 = (1 << 32) - 1
BUCKET = 4                     # SCONE_BUCKET: slots per bucket
UNI_CAP = 1 << 18              # SCONE_UNI_CAP: unigram tokens below this resolve through the direct table
TOKEN_LIMIT_N4 = 0xFFFFFF      # max_n = 4 stores token + 1 in 24 bits: tokens >= 2^24 - 1 cannot be keys
MAX_BATCH_TOKENS = 6200


# ------------------------------------------------------------------ the functions of scone_common.h
def pack_key(tokens, max_n):
    """(ok, lo, ext) of the f-gram `tokens` (1 .. max_n unsigned 32-bit ids).  Tokens are stored + 1.  max_n <= 3: 32 bits per
    token, lo = v0 | v1 << 32, ext = v2.  max_n = 4: 24 bits per token, lo = v0 | v1 << 24 | (v2 & 0xFFFF) << 48,
    ext = v2 >> 16 | v3 << 8.  `ok` is False where a token cannot be represented (the other two fields then hold what the
    product's arithmetic leaves in them)."""
    n = len(tokens)
    t = [int(x) for x in tokens]
    if max_n <= 3:
        v = [t[i] + 1 if i < n else 0 for i in range(3)]
        ok = all((x >> 32) == 0 for x in v)
        lo = (v[0] | (v[1] << 32)) & M64
        ext = v[2] & M32
    else:
        v = [(t[i] + 1) & M32 if i < n else 0 for i in range(4)]
        ok = all(x < TOKEN_LIMIT_N4 for x in t)
        lo = (v[0] | (v[1] << 24) | ((v[2] & 0xFFFF) << 48)) & M64
        ext = ((v[2] >> 16) | (v[3] << 8)) & M32
    return ok, lo, ext


def hash_key(lo, ext):
    x = lo ^ ((ext * 0x9E3779B97F4A7C15) & M64)
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & M64
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & M64
    x ^= x >> 31
    return x


def bucket_home(h, slot_mask):
    return h & (slot_mask >> 2)


def bucket_step(h):
    return (h >> 32) | 1


def bloom_bit(h, bloom_mask):
    return (h >> 20) & bloom_mask


def bloom_bits(capacity):
    """Size of the presence bitmap of an index of `capacity` slots (scone_create): 8 bits per slot within [1024, 2^30]."""
    return min(max(8 * capacity, 1024), 1 << 30)


# ------------------------------------------------------------------ order-independent facts of a built index
def key_hash(tokens, max_n):
    ok, lo, ext = pack_key(tokens, max_n)
    assert ok, tokens
    return hash_key(lo, ext)


def distinct_keys(keys, lens):
    """{f-gram tuple: smallest id}, ids = row numbers."""
    out = {}
    for i in range(len(lens)):
        out.setdefault(tuple(int(x) for x in keys[i, :lens[i]]), i)
    return out


def homed(distinct, max_n, capacity):
    """Counter {bucket: distinct keys whose probe sequence starts there}."""
    return collections.Counter(bucket_home(key_hash(g, max_n), capacity - 1) for g in distinct)


def bitmap(distinct, max_n, capacity):
    """The set bits of the presence bitmap."""
    mask = bloom_bits(capacity) - 1
    return {bloom_bit(key_hash(g, max_n), mask) for g in distinct}


def bit_is_set(g, bits, max_n, capacity):
    ok, lo, ext = pack_key(g, max_n)
    return ok and bloom_bit(hash_key(lo, ext), bloom_bits(capacity) - 1) in bits


# ------------------------------------------------------------------ batches
Batch = collections.namedtuple("Batch", "rect packed cu")     # [B, T] int64; [total] int64; [n_seqs + 1] int64


def sequences(batch, form):
    if form == "rect":
        return [row for row in batch.rect]
    return [batch.packed[batch.cu[s]:batch.cu[s + 1]] for s in range(len(batch.cu) - 1)]


def windows(seqs, max_n):
    """Counter of the windows (length 1 .. max_n, inside one sequence, no negative token) that a matcher forms."""
    out = collections.Counter()
    for seq in seqs:
        s = [int(x) for x in seq]
        for i in range(len(s)):
            for n in range(1, max_n + 1):
                if i + n > len(s) or s[i + n - 1] < 0:
                    break
                out[tuple(s[i:i + n])] += 1
    return out


PACKED_BUDGETS = (37, 0, 1, 700, 2, 255, 256, 257, 90, 3, 513, 129, 5, 64)


def _layout(items, rng, filler, T):
    """The token tuples `items` (shuffled), each whole inside one sequence, as a rectangle of rows of T tokens and as a packed
    stream whose sequences close where the next item no longer fits a budget from PACKED_BUDGETS (0: an empty sequence).  Between
    two items: nothing, a filler token or -1."""
    items = [tuple(int(x) for x in it) for it in items]
    order = rng.permutation(len(items))
    items = [items[i] for i in order]
    assert max(len(it) for it in items) <= min(T, max(PACKED_BUDGETS))

    def gap():
        r = rng.random()
        return [] if r < 0.4 else ([-1] if r < 0.7 else [int(filler[rng.integers(len(filler))])])

    rows, cur = [], []
    for it in items:
        g = gap()
        if len(cur) + len(g) + len(it) > T:
            rows.append(cur)
            cur, g = [], []
        cur += g + list(it)
    rows.append(cur)
    rect = np.full((len(rows), T), -1, dtype=np.int64)
    for r, row in enumerate(rows):
        rect[r, :len(row)] = row
        for j in range(len(row), T):                      # the rest of the row: fillers and -1
            rect[r, j] = -1 if rng.random() < 0.3 else int(filler[rng.integers(len(filler))])
    seqs, cur, b = [], [], 0
    for it in items:
        g = gap()
        while len(cur) + len(g) + len(it) > PACKED_BUDGETS[b % len(PACKED_BUDGETS)]:
            seqs.append(cur)
            cur, g = [], []
            b += 1
        cur += g + list(it)
    seqs += [cur, [], [-1], [int(filler[0])]]
    cu = np.zeros(len(seqs) + 1, dtype=np.int64)
    np.cumsum([len(s) for s in seqs], out=cu[1:])
    packed = np.asarray([x for s in seqs for x in s], dtype=np.int64)
    return Batch(rect, packed, cu)


def _batch_facts(batch, max_n, dist):
    """What every batch promises, per form, and the windows it holds."""
    facts = {}
    win = {}
    for form in ("rect", "packed"):
        seqs = sequences(batch, form)
        win[form] = windows(seqs, max_n)
        facts[f"{form}_tokens"] = int(sum(len(s) for s in seqs))
        facts[f"{form}_sequences"] = len(seqs)
        facts[f"{form}_minus_one_tokens"] = int(sum(int((np.asarray(s) < 0).sum()) for s in seqs))
        facts[f"{form}_present_windows"] = int(sum(c for g, c in win[form].items() if g in dist))
        facts[f"{form}_absent_windows"] = int(sum(c for g, c in win[form].items() if g not in dist))
    facts["keys_missing_from_batch"] = sum(1 for g in dist if not _in_both(win, g))
    lens = np.diff(batch.cu)
    facts["packed_empty_sequences"] = int((lens == 0).sum())
    facts["packed_distinct_lengths"] = len(set(lens.tolist()))
    return facts, win


def _in_both(win, g):
    return min(win["rect"][g], win["packed"][g])


def _arrays(rows, max_n):
    keys = np.zeros((len(rows), max_n), dtype=np.uint32)
    lens = np.zeros(len(rows), dtype=np.uint8)
    for i, g in enumerate(rows):
        keys[i, :len(g)] = g
        lens[i] = len(g)
    return keys, lens


def _thirds(n):
    return [0, n // 3, 2 * n // 3, n]


def _random_key(rng, max_n, n=None, wide=0.1):
    """Tokens mostly below 60,000, now and then at or above 2^18 (below 2^20: packable in both layouts)."""
    n = int(rng.integers(1, max_n + 1)) if n is None else n
    return tuple(int(rng.integers(UNI_CAP, 1 << 20)) if rng.random() < wide else int(rng.integers(0, 60000)) for _ in range(n))


# ------------------------------------------------------------------ crowded
CROWDED_BUCKETS, CROWDED_KEYS = 8, 12


def crowded(max_n, capacity=1024):
    """Load ~0.75 with CROWDED_BUCKETS buckets that are each the home of >= CROWDED_KEYS distinct keys (a bucket holds 4: the rest
    sit further along their step sequence, whatever the insertion order), found by rejection sampling with the model."""
    rng = np.random.default_rng(1000 + max_n)
    nb = capacity // BUCKET
    targets = [int(b) for b in rng.choice(nb, size=CROWDED_BUCKETS, replace=False)]
    got = {b: [] for b in targets}
    seen = set()
    while any(len(v) < CROWDED_KEYS + 1 for v in got.values()):
        g = _random_key(rng, max_n)
        if g in seen:
            continue
        b = bucket_home(key_hash(g, max_n), capacity - 1)
        if b in got and len(got[b]) < CROWDED_KEYS + 1:
            got[b].append(g)
            seen.add(g)
    crowd = [g for v in got.values() for g in v]
    rows = list(crowd)
    while len(rows) < (3 * capacity) // 4:
        g = _random_key(rng, max_n)
        if g not in seen:
            seen.add(g)
            rows.append(g)
    rows = [rows[i] for i in rng.permutation(len(rows))]
    keys, lens = _arrays(rows, max_n)
    dist = distinct_keys(keys, lens)
    hc = homed(dist, max_n, capacity)
    big = {b for b, c in hc.items() if c >= CROWDED_KEYS}
    big_keys = [g for g in dist if bucket_home(key_hash(g, max_n), capacity - 1) in big]
    ordinary = [g for g in rows if g not in set(big_keys)]
    absent = []
    while len(absent) < 200:
        g = _random_key(rng, max_n)
        if g not in dist:
            absent.append(g)
    # absent keys that share all but the last token with a crowded key
    near = [g[:-1] + ((g[-1] + 1) % 60000,) for g in big_keys if g[:-1] + ((g[-1] + 1) % 60000,) not in dist]
    items = big_keys + ordinary + absent + near          # every key: wherever the build put it, it must be found there
    batch = _layout(items, rng, filler=[t for g in ordinary[:64] for t in g], T=300)
    facts, win = _batch_facts(batch, max_n, dist)
    facts.update(n_rows=len(rows), n_distinct=len(dist), load=len(dist) / capacity,
                 crowded_buckets=len(big), crowded_min_keys=min(hc[b] for b in big) if big else 0,
                 keys_beyond_their_home_at_least=sum(hc[b] - BUCKET for b in big),
                 crowded_keys=len(big_keys), crowded_keys_missing_from_batch=sum(1 for g in big_keys if _in_both(win, g) == 0),
                 chunk_bounds=_thirds(len(rows)))
    return keys, lens, capacity, batch, facts


# ------------------------------------------------------------------ full
FULL_CAPACITIES = (4, 64, 1024)
FULL_FALSE_POSITIVES, FULL_PRESENT_PER_LENGTH = 32, 32


def full(max_n, capacity):
    """Exactly `capacity` distinct keys of lengths 1 .. max_n: no slot is empty, so an absent key that passes the bitmap (a false
    positive, found with the model) walks all capacity / 4 buckets and stops on the try count.  The batch holds every key."""
    rng = np.random.default_rng(2000 + 10 * capacity + max_n)
    vocab = [int(x) for x in rng.choice(50000, size=40, replace=False)] + [UNI_CAP - 1, UNI_CAP, UNI_CAP + 1, (1 << 20) + 3,
                                                                          (1 << 19) + 7, (1 << 18) + 4099, (1 << 21) + 1, (1 << 22) + 5]
    per = [capacity // max_n] * max_n
    per[0] = min(per[0], len(vocab) // 2)
    per[-1] += capacity - sum(per)
    rows, seen = [], set()
    for n in range(1, max_n + 1):
        have = 0
        while have < per[n - 1]:
            g = tuple(vocab[int(i)] for i in rng.integers(0, len(vocab), size=n))
            if g not in seen:
                seen.add(g)
                rows.append(g)
                have += 1
    rows = [rows[i] for i in rng.permutation(len(rows))]
    keys, lens = _arrays(rows, max_n)
    dist = distinct_keys(keys, lens)
    bits = bitmap(dist, max_n, capacity)
    fp, fp_uni = [], []
    while len(fp) < FULL_FALSE_POSITIVES + 8:            # absent, length >= 2, bitmap bit set
        n = int(rng.integers(2, max_n + 1))
        g = tuple(vocab[int(rng.integers(len(vocab)))] if rng.random() < 0.3 else int(rng.integers(0, 1 << 20)) for _ in range(n))
        if g not in dist and g not in fp and bit_is_set(g, bits, max_n, capacity):
            fp.append(g)
    while len(fp_uni) < 8:                               # absent unigrams the direct table does not answer, bitmap bit set
        g = (int(rng.integers(UNI_CAP, 1 << 22)),)
        if g not in dist and g not in fp_uni and bit_is_set(g, bits, max_n, capacity):
            fp_uni.append(g)
    items = fp + fp_uni
    for n in range(1, max_n + 1):
        mine = [g for g in rows if len(g) == n]
        items += [mine[int(i)] for i in rng.integers(0, len(mine), size=FULL_PRESENT_PER_LENGTH + 8)]
    items += rows                                        # every key: wherever the build put it, some matcher must find it there
    items += [tuple(vocab[int(i)] for i in rng.integers(0, len(vocab), size=max_n)) for _ in range(150)]
    batch = _layout(items, rng, filler=vocab, T=257)
    facts, win = _batch_facts(batch, max_n, dist)
    both = {g: _in_both(win, g) for g in set(win["rect"]) | set(win["packed"])}
    facts.update(n_rows=len(rows), n_distinct=len(dist), capacity=capacity, buckets=capacity // BUCKET,
                 lengths_present=sorted({len(g) for g in dist}),
                 false_positive_absent_windows=sum(1 for g, c in both.items()
                                                   if c and len(g) >= 2 and g not in dist and bit_is_set(g, bits, max_n, capacity)),
                 false_positive_absent_wide_unigrams=sum(1 for g, c in both.items()
                                                         if c and len(g) == 1 and g[0] >= UNI_CAP and g not in dist
                                                         and bit_is_set(g, bits, max_n, capacity)),
                 present_windows_per_length=[sum(c for g, c in both.items() if len(g) == n and g in dist) for n in range(1, max_n + 1)],
                 chunk_bounds=_thirds(len(rows)))
    return keys, lens, capacity, batch, facts


# ------------------------------------------------------------------ shared lo
SHARED_PAIRS = 64


def shared_lo(max_n, capacity=512):
    """Present and absent keys that differ only in `ext` (the comparison `scan_bucket` / `resolve_queue` make AFTER lo matched).
    max_n = 3: trigram (a, b, c) present, (a, b, c') absent; the bigram (a, b) -- same lo, ext = 0 -- is present in one half of
    the groups and absent in the other.  max_n = 4: keys that agree in tokens 0 and 1 and in the low 16 bits of token 2 + 1 --
    kind A: the trigram (a, b, c) present, (a, b, c + 65,536 k) absent; kind B: (a, b, c, e) present, (a, b, c, e') absent, the
    trigram (a, b, c) present in one half of the groups and absent in the other.  Every absent key named here is one whose
    bitmap bit is set (picked with the model).  max_n = 2 has no such state: ext is 0 for every key of that layout."""
    if max_n < 3:
        raise ValueError("at max_n <= 2 every key has ext = 0: no two keys share lo")
    rng = np.random.default_rng(3000 + max_n)
    n_groups = 96
    rows, seen = [], set()

    def add(g):
        if g not in seen:
            seen.add(g)
            rows.append(g)

    def tok():
        return int(rng.integers(0, 3000))

    def shorter(a, b, c):
        return (a, b) if max_n == 3 else (a, b, c)

    def add_group(a, b, c, kind, with_shorter):
        if max_n == 3:
            add((a, b, c))
            add((a, b, int(rng.integers(3000, 6000))))   # a second present trigram of the same lo
        elif kind == "A":
            add((a, b, c))
            add((a, b, c + 65536 * 255))                  # a second present trigram of the same lo
        else:
            add((a, b, c, tok()))
            add((a, b, c, int(rng.integers(3000, 6000))))
        if with_shorter:
            add(shorter(a, b, c))

    for _ in range(60):
        add(_random_key(rng, max_n, wide=0.05))
    groups = []                                           # (a, b, c, kind, shorter key present / absent / not applicable)
    for i in range(n_groups // 2):
        kind = "A" if (max_n == 4 and i % 3 == 0) else "B"
        a, b, c = tok(), tok(), tok()
        groups.append((a, b, c, kind, None if kind == "A" else True))
        add_group(a, b, c, kind, kind == "B")
    bits = bitmap({g: 0 for g in rows}, max_n, capacity)  # bits are only ever added: what is set now stays set
    for i in range(n_groups // 2):
        kind = "A" if (max_n == 4 and i % 3 == 0) else "B"
        while True:
            a, b, c = tok(), tok(), tok()
            if kind == "A" or (shorter(a, b, c) not in seen and bit_is_set(shorter(a, b, c), bits, max_n, capacity)):
                break
        groups.append((a, b, c, kind, None if kind == "A" else False))
        add_group(a, b, c, kind, False)
    rows = [rows[i] for i in rng.permutation(len(rows))]
    keys, lens = _arrays(rows, max_n)
    dist = distinct_keys(keys, lens)
    bits = bitmap(dist, max_n, capacity)
    pairs, shorter_absent = [], []
    for a, b, c, kind, with_shorter in groups:
        p = (a, b, c) if (max_n == 3 or kind == "A") else next(g for g in rows if g[:3] == (a, b, c) and len(g) == 4)
        while True:                                       # an absent partner that differs only in ext and passes the bitmap
            if max_n == 3:
                q = (a, b, int(rng.integers(0, 1 << 20)))
            elif kind == "A":
                q = (a, b, c + 65536 * int(rng.integers(1, 255)))
            else:
                q = (a, b, c, int(rng.integers(0, 1 << 20)))
            if q not in dist and bit_is_set(q, bits, max_n, capacity):
                pairs.append((p, q))
                break
        if with_shorter is False:
            shorter_absent.append(shorter(a, b, c))
    items = [g for pq in pairs for g in pq] + shorter_absent + rows
    batch = _layout(items, rng, filler=[tok() for _ in range(64)], T=257)
    facts, win = _batch_facts(batch, max_n, dist)

    def differ_only_in_ext(p, q):
        (_, plo, pext), (_, qlo, qext) = pack_key(p, max_n), pack_key(q, max_n)
        return plo == qlo and pext != qext

    good = [(p, q) for p, q in pairs if p in dist and q not in dist and differ_only_in_ext(p, q)
            and bit_is_set(q, bits, max_n, capacity) and _in_both(win, p) and _in_both(win, q)]
    facts.update(n_rows=len(rows), n_distinct=len(dist), load=len(dist) / capacity, pairs=len(good),
                 pairs_token2_moved_by_65536=sum(1 for p, q in good if max_n == 4 and len(p) == 3),
                 pairs_last_token_differs=sum(1 for p, q in good if len(p) == max_n),
                 shorter_key_present=sum(1 for a, b, c, k, w in groups if w is True and shorter(a, b, c) in dist
                                         and _in_both(win, shorter(a, b, c))),
                 shorter_key_absent_bit_set=sum(1 for g in shorter_absent if g not in dist and bit_is_set(g, bits, max_n, capacity)
                                                and _in_both(win, g)),
                 chunk_bounds=_thirds(len(rows)))
    return keys, lens, capacity, batch, facts


# ------------------------------------------------------------------ wide tokens
WIDE_RUN = 600


def wide_tokens(max_n):
    return [UNI_CAP - 1, UNI_CAP, UNI_CAP + 1, (1 << 20) + 3, (1 << 24) - 2 if max_n == 4 else (1 << 31) - 1]


def unpackable_tokens(max_n):
    """Tokens of the batch that no key can hold (max_n = 4 only; at max_n <= 3 every int32 token packs)."""
    return [(1 << 24) - 1, (1 << 31) - 1] if max_n == 4 else []


def wide(max_n, capacity=512):
    """Keys over token ids around and far above 2^18 (unigrams at or above 2^18 are the only ones that go to the hash table), the
    same tokens moved by one as absent tokens, and one run `a b a b ...` of > WIDE_RUN tokens over two wide tokens whose
    unigrams, bigrams, ... are all keys: every window start of a whole k_match_ell tile queues max_n probes."""
    rng = np.random.default_rng(4000 + max_n)
    W = wide_tokens(max_n)
    top = TOKEN_LIMIT_N4 if max_n == 4 else (1 << 31)
    off = sorted({t + s for t in W for s in (-1, 1)} - set(W))
    off = [t for t in off if t < top]
    a, b = UNI_CAP, (1 << 20) + 3
    rows, seen = [], set()

    def add(g):
        if g not in seen:
            seen.add(g)
            rows.append(g)

    for t in W:
        add((t,))
    for n in range(1, max_n + 1):                         # every window of the run
        add(tuple((a, b)[j % 2] for j in range(n)))
        add(tuple((b, a)[j % 2] for j in range(n)))
    for n in range(2, max_n + 1):
        for _ in range(60):
            add(tuple(W[int(i)] for i in rng.integers(0, len(W), size=n)))
        add(tuple([W[-1]] * n))                           # the top token in every place
    for _ in range(40):                                   # ordinary small keys next to them
        add(_random_key(rng, max_n, wide=0.0))
    rows = [rows[i] for i in rng.permutation(len(rows))]
    keys, lens = _arrays(rows, max_n)
    dist = distinct_keys(keys, lens)
    run = tuple((a, b)[j % 2] for j in range(WIDE_RUN + 40))
    items = [run]
    pool = W * 3 + off + unpackable_tokens(max_n)
    for _ in range(260):                                  # walks over present, absent and unpackable tokens
        items.append(tuple(pool[int(i)] for i in rng.integers(0, len(pool), size=int(rng.integers(1, 9)))))
    items += rows
    batch = _layout(items, rng, filler=W + off, T=704)
    facts, win = _batch_facts(batch, max_n, dist)
    facts.update(n_rows=len(rows), n_distinct=len(dist), load=len(dist) / capacity,
                 saturated_run=min(max(_longest_saturated_run(q, dist, max_n) for q in sequences(batch, f)) for f in ("rect", "packed")),
                 wide_tokens_as_unigram_keys=sum(1 for t in W if (t,) in dist),
                 wide_unigram_windows_at_or_above_2_18=sum(_in_both(win, (t,)) for t in W if t >= UNI_CAP),
                 absent_tokens_in_batch=sum(1 for t in off if _in_both(win, (t,)) and (t,) not in dist),
                 unpackable_tokens_in_batch=sum(1 for t in unpackable_tokens(max_n)
                                                if (batch.rect == t).any() and (batch.packed == t).any()),
                 boundary_tokens_in_keys=sorted({t for g in dist for t in g if t in W}),
                 chunk_bounds=_thirds(len(rows)))
    return keys, lens, capacity, batch, facts


def _longest_saturated_run(seq, dist, max_n):
    """Longest run of consecutive positions of `seq` at which EVERY window of length 1 .. max_n that starts there is a key made
    of tokens >= 2^18 (so the start queues max_n probes: its unigram included) -- counted up to the last start whose longest
    window still fits."""
    s = [int(x) for x in seq]
    best = cur = 0
    for i in range(len(s) - max_n + 1):
        ok = all(s[i + j] >= UNI_CAP for j in range(max_n)) and all(tuple(s[i:i + n]) in dist for n in range(1, max_n + 1))
        cur = cur + 1 if ok else 0
        best = max(best, cur)
    return best


# ------------------------------------------------------------------ duplicates
def duplicates(max_n, capacity=1024):
    """The same key under several ids that lie in different build chunks (`facts["chunk_bounds"]`), unigrams on both sides of
    2^18 among them: the smallest id wins, in the hash table and in the direct unigram table, whatever the chunk order."""
    rng = np.random.default_rng(5000 + max_n)
    per_chunk = 220
    uni_small = [(int(t),) for t in rng.choice(50000, size=24, replace=False)] + [(UNI_CAP - 1,), (0,)]
    uni_wide = [(UNI_CAP,), (UNI_CAP + 1,), ((1 << 20) + 3,), ((1 << 22) + 9,)] + [(int(rng.integers(UNI_CAP, 1 << 23)),) for _ in range(8)]
    longer = []
    while len(longer) < 110:
        g = _random_key(rng, max_n, n=int(rng.integers(2, max_n + 1)))
        if g not in longer:
            longer.append(g)
    dup = list(dict.fromkeys(uni_small + uni_wide + longer))
    chunks = [[], [], []]
    for k, g in enumerate(dup):
        where = [(0, 1), (1, 2), (0, 2), (0, 1, 2), (2, 1), (1, 2)][k % 6]
        for c in where:
            chunks[c].append(g)
        if k % 7 == 0:
            chunks[where[-1]].append(g)                   # and twice inside one chunk
    seen = set(dup)
    for c in range(3):
        assert len(chunks[c]) <= per_chunk
        while len(chunks[c]) < per_chunk:
            g = _random_key(rng, max_n)
            if g not in seen:
                seen.add(g)
                chunks[c].append(g)
        chunks[c] = [chunks[c][i] for i in rng.permutation(per_chunk)]
    rows = chunks[0] + chunks[1] + chunks[2]
    keys, lens = _arrays(rows, max_n)
    dist = distinct_keys(keys, lens)
    bounds = [0, per_chunk, 2 * per_chunk, 3 * per_chunk]
    ids = collections.defaultdict(list)
    for i, g in enumerate(rows):
        ids[g].append(i)
    multi = {g: v for g, v in ids.items() if len(v) > 1}

    def chunk_of(i):
        return i // per_chunk

    absent = []
    while len(absent) < 100:
        g = _random_key(rng, max_n)
        if g not in dist:
            absent.append(g)
    singles = [g for g in rows if g not in multi]
    items = list(multi) + singles + absent
    batch = _layout(items, rng, filler=[t for g in singles[:64] for t in g], T=300)
    facts, win = _batch_facts(batch, max_n, dist)
    facts.update(n_rows=len(rows), n_distinct=len(dist), n_dups=len(rows) - len(dist), duplicated_keys=len(multi),
                 duplicated_keys_in_several_chunks=sum(1 for v in multi.values() if len({chunk_of(i) for i in v}) > 1),
                 duplicated_keys_smallest_id_not_in_chunk_0=sum(1 for v in multi.values() if chunk_of(min(v)) > 0),
                 duplicated_keys_smallest_id_not_in_chunk_2=sum(1 for v in multi.values() if chunk_of(min(v)) < 2),
                 duplicated_unigrams_below_2_18=sum(1 for g in multi if len(g) == 1 and g[0] < UNI_CAP),
                 duplicated_unigrams_at_or_above_2_18=sum(1 for g in multi if len(g) == 1 and g[0] >= UNI_CAP),
                 duplicated_keys_missing_from_batch=sum(1 for g in multi if _in_both(win, g) == 0),
                 chunk_bounds=bounds)
    return keys, lens, capacity, batch, facts


# ------------------------------------------------------------------ the list of states
def states():
    """[(name, generator, max_n, capacity argument or None)]: every generator at max_n 2, 3, 4 (`full` at its three capacities;
    `shared_lo` at 3 and 4: the max_n <= 3 layout has ext = 0 for every key of length <= 2)."""
    out = []
    for max_n in (2, 3, 4):
        out.append((f"crowded-n{max_n}", crowded, max_n, None))
        for cap in FULL_CAPACITIES:
            out.append((f"full{cap}-n{max_n}", full, max_n, cap))
        if max_n >= 3:
            out.append((f"shared_lo-n{max_n}", shared_lo, max_n, None))
        out.append((f"wide-n{max_n}", wide, max_n, None))
        out.append((f"duplicates-n{max_n}", duplicates, max_n, None))
    return out


_CACHE = {}


def state(name):
    """The state `name` of states(), generated once per process."""
    if name not in _CACHE:
        for nm, gen, max_n, cap in states():
            if nm == name:
                _CACHE[name] = (max_n,) + (gen(max_n) if cap is None else gen(max_n, cap))
    return _CACHE[name]
