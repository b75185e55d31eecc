"""Which calls tests/test_gpu_call_sequences.py puts behind which on one handle, as plain Python (no GPU): the rings of
every arena, the two shuffles of the whole table, the scale sequences and the pairs of the stream-order test.

A handle's scratch is nine reused arenas and two device copies of kernel scales; in production the call before any call
is some other entry point.  The property the GPU tests hold every plan element to: a clean call returns, bit for bit,
what the same call returns alone on a fresh handle, whatever went through the handle before it.

Everything here is a function of tests/contract_table.py alone.  Where an order is random it is seeded with
`zlib.crc32` of a fixed tag (str hashes are salted per process): two processes -- the collection of a parallel run, a
rerun of one failing id -- see the same plan."""

import zlib

import numpy as np

import contract_table as ct

SLICE = 40           # elements of a shuffle that share one handle
SHUFFLES = 2
GENERIC_D_ROWS = ("mgp_k_dense", "mgp_nearest_center", "mgp_k_dense_vjp", "mgp_kmn_knm_vjp_anyd",
                  "mgp_k_dense_vjp_points", "mgp_knm_matvec")  # rows with a case at D = 33 that upload h->dparams
STREAM_ROWS = ("mgp_knm_matvec", "mgp_kmn_matvec_anyd", "mgp_knm_quadform", "mgp_rff_sample")  # all asynchronous


def seed(*tag):
    return zlib.crc32(repr(tag).encode()) & 0x7FFFFFFF


def triples(table=None):
    """every (row name, case index, dtype) of the table, in table order"""
    table = ct.TABLE if table is None else table
    return [(r.name, ci, dt) for r in table for ci in range(len(r.cases)) for dt in r.dtypes]


# ---------------------------------------------------------------------------------------------------- rings
def ring(arena, table=None):
    """the rows whose `arenas` list `arena`, in table order; row i is read behind row i + 1 (cyclically)"""
    table = ct.TABLE if table is None else table
    return [r.name for r in table if arena in r.arenas]


def ring_pairs(arena, table=None):
    """[(reader, writer)]: the writer's poison run stands between the reader's two clean runs"""
    names = ring(arena, table)
    return [(names[i], names[(i + 1) % len(names)]) for i in range(len(names))]


def writer_dtype(writer, dt):
    """the reader's dtype where the writer has it, else the writer's only one"""
    return dt if dt in writer.dtypes else writer.dtypes[0]


def writer_cases(arena, reader, ci, dt, writer):
    """the order in which the writer's cases are tried as poison until the library reports `arena` held: a rotation of
    the writer's cases whose start depends on the reader's case, so that the pairs of a ring differ"""
    n = len(writer.cases)
    start = seed("ring", arena, reader, ci, dt, writer.name) % n
    return [(start + i) % n for i in range(n)]


def ring_items(table=None):
    """[(arena, reader name, case index, dtype, writer name)] for every arena, every reader and each of its cases"""
    table = ct.TABLE if table is None else table
    by_name = {r.name: r for r in table}
    out = []
    for arena in ct.ARENAS:
        for reader, writer in ring_pairs(arena, table):
            row = by_name[reader]
            out += [(arena, reader, ci, dt, writer) for ci in range(len(row.cases)) for dt in row.dtypes]
    return out


# ---------------------------------------------------------------------------------------------------- shuffles
def shuffle(k, table=None):
    """the k-th seeded permutation of all triples"""
    t = triples(table)
    order = np.random.default_rng(seed("shuffle", k, len(t))).permutation(len(t))
    return [t[i] for i in order]


def shuffle_slices(table=None):
    """[(k, slice index, [(element, predecessor)])]: an element is a triple, its predecessor the element before it in
    the permutation (cyclically: the first of a slice follows the last of the slice before), whose row's poison run
    precedes the element's clean run"""
    out = []
    for k in range(SHUFFLES):
        perm = shuffle(k, table)
        pairs = [(perm[i], perm[i - 1]) for i in range(len(perm))]
        out += [(k, s // SLICE, pairs[s:s + SLICE]) for s in range(0, len(pairs), SLICE)]
    return out


# ---------------------------------------------------------------------------------------------------- scales
def d33_case(row):
    """index of the row's first case at D = 33"""
    return next(i for i, c in enumerate(row.cases) if c.get("D") == 33)


def generic_d_pairs():
    """[(first, second)] over the generic-D rows: first, second with other lengthscales, first again"""
    return [(a, b) for a in GENERIC_D_ROWS for b in GENERIC_D_ROWS if a != b]


def other_lengthscales(ls):
    """lengthscales no call of the table uses: every entry changed, none by a power of two"""
    ls = np.asarray(ls, dtype=np.float64)
    return ls * np.linspace(1.31, 0.71, ls.shape[0])  # the midpoint is 1.01: no factor is 1


# ---------------------------------------------------------------------------------------------------- streams
def stream_pairs(table=None):
    """[(X, Y, shared arenas)]: X is enqueued on one stream behind producers, Y through the same handle on another.
    mgp_knm_quadform lists `prj` alone, which none of the other three reaches: its pairs share the handle, whose calls
    the contract orders whatever they touch, and no arena (the tuple is empty)."""
    table = ct.TABLE if table is None else table
    by_name = {r.name: r for r in table}
    return [(x, y, tuple(a for a in ct.ARENAS if a in by_name[x].arenas and a in by_name[y].arenas))
            for x in STREAM_ROWS for y in STREAM_ROWS if x != y]


STREAM_CASE = {"mgp_knm_matvec": 1, "mgp_kmn_matvec_anyd": 2, "mgp_knm_quadform": 1, "mgp_rff_sample": 0}


def counts(table=None):
    """the figures DESIGN.md quotes"""
    items = ring_items(table)
    slices = shuffle_slices(table)
    per_arena = {a: (len(ring(a, table)), sum(1 for it in items if it[0] == a)) for a in ct.ARENAS}
    return dict(triples=len(triples(table)), rings=per_arena, ring_items=len(items), slices=len(slices),
                shuffle_calls=2 * sum(len(s[2]) for s in slices), generic_d_pairs=len(generic_d_pairs()),
                stream_pairs=len(stream_pairs(table)))
