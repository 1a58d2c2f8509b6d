"""Recorder of the exact-inference passes (embed_full / predict_full, embed_nodes / predict_nodes, rank_full, topk_full) as the HOST
code of one checkout drives them, at the small seeded shapes of tests/infer_cases.py.

    GS_LIB=<in-tree library> python tests/golden/make_infer_parent_outputs.py --tree <checkout to pin>     # on the GPU

puts <checkout>/ first on sys.path before graphsage_amd is imported, so that checkout's Python drives the library GS_LIB names,
and writes tests/golden/infer_parent_outputs.npz.  Only calls every checkout since embed_nodes / topk_full has are used:
embed_full, predict_full, embed_nodes, predict_nodes, rank_full, topk_full, FullGraph, inference.WINDOW_ROWS.  The inputs are not
stored: `run(name)` rebuilds them from the seeds of infer_cases.  tests/test_infer_golden_gpu.py recomputes every case with the
in-tree package and compares float outputs as float values, with no tolerance, and integer outputs with array_equal.

The file in the tree was recorded with the Python of commit ed07ca9 ("Importance neighborhoods: walk visit counts as the sampler's
table") -- the last commit in which every aggregator stated its full-neighborhood layer twice (infer_full and infer_rows) and
rank_full / topk_full each carried their own query prelude -- driving the library of the commit that added this file (the two
build the same library: nothing under csrc/ or include/ differs).  Regenerate it only when the launch sequence of these passes
is meant to change, and say so in the commit.

Stored per output `<case>.<output>` (`index`, JSON): the array itself when it has at most 8 KB (a slice of `whole`, or of
`whole_int` for an integer output); else the SHA-256 of its bytes with -0 folded to +0, so that equal float VALUES hash alike (a
row of `sha256`).  An output whose bytes equal those of an output stored earlier is a `same_as` entry naming that one.

Cases, one per model (the ten MODELS of infer_cases and `unsup_bilinear` = the unsupervised mean model at dim 32 with bilinear_weights=True), N = 300,
F = 20, a hub of 2 SPLIT_LEN + 77 edges cut in three, an isolated node:
  every one of the ten, over the CSR graph:
    full.emb / full.preds              embed_full / predict_full
    <request>.emb / <request>.preds    embed_nodes / predict_nodes for the requests many (17 ids, one twice), hub, isolated
  mean_narrow, gcn_narrow, gcn_plain, maxpool, twomaxpool:
    win16.emb / win16.preds            the whole-graph pass with inference.WINDOW_ROWS = 16: 19 windows, the last of 13 rows
  mean_narrow, maxpool:
    padded.emb / padded.preds          the subset pass for many + the isolated node on the padded graph (no cut row)
  unsup_mean, unsup_bilinear, with the filter on (`filt`) and off (`raw`):
    rank_<f>.n_gt / n_eq / scores      rank_full on 40 seeded edges
    topk_<f>.ids / scores / count      topk_full with k = 5 for the 17 ids of many"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN_FILE = os.path.join(HERE, "infer_parent_outputs.npz")
WHOLE_BYTES = 8 * 1024
BILINEAR = "unsup_bilinear"
WINDOWED = ("mean_narrow", "gcn_narrow", "gcn_plain", "maxpool", "twomaxpool")
PADDED = ("mean_narrow", "maxpool")
RANKED = ("unsup_mean", BILINEAR)
REQUESTS = ("many", "hub", "isolated")


def _cases():
    tests = os.path.dirname(HERE)
    if tests not in sys.path:
        sys.path.insert(0, tests)
    import infer_cases
    return infer_cases


def case_names():
    return tuple(sorted(_cases().MODELS)) + (BILINEAR,)


def run(name):
    """The case through the importable graphsage_amd -> {output name: array}."""
    ic = _cases()
    from graphsage_amd import inference as inf
    model = ic.build(name)[0]
    graphs = ic.world()["graphs"]
    graph = graphs["csr"][0]
    res = {}

    def put(key, out):
        res[key + ".emb"] = out[0]
        if hasattr(model, "predict_full"):
            res[key + ".preds"] = out[1]

    def full():
        return model.predict_full(graph) if hasattr(model, "predict_full") else (model.embed_full(graph),)

    def nodes(g, ids):
        return model.predict_nodes(g, ids) if hasattr(model, "predict_nodes") else model.embed_nodes(g, ids)

    many = ic.many_request()
    if name != BILINEAR:
        put("full", full())
        for what, ids in zip(REQUESTS, (many, [ic.HUB], [ic.ISOLATED])):
            put(what, nodes(graph, ids))
    if name in WINDOWED:
        keep, inf.WINDOW_ROWS = inf.WINDOW_ROWS, 16
        try:
            put("win16", full())
        finally:
            inf.WINDOW_ROWS = keep
    if name in PADDED:
        put("padded", nodes(graphs["padded"][0], many + [ic.ISOLATED]))
    if name in RANKED:
        edges = np.random.RandomState(7).randint(0, ic.N, size=(40, 2))
        for f, filtered in (("filt", True), ("raw", False)):
            r = model.rank_full(graph, edges, filtered=filtered)
            t = model.topk_full(graph, many, k=5, filtered=filtered)
            res.update({"rank_%s.n_gt" % f: r["n_gt"], "rank_%s.n_eq" % f: r["n_eq"], "rank_%s.scores" % f: r["scores"],
                        "topk_%s.ids" % f: t["ids"], "topk_%s.scores" % f: t["scores"], "topk_%s.count" % f: t["count"]})
    return res


def is_int(a):
    return np.issubdtype(a.dtype, np.integer)


def fold(a):
    """The array's bytes with -0 folded to +0."""
    return np.where(a == 0, np.zeros((), a.dtype), a).tobytes()


def digest(a):
    return np.frombuffer(hashlib.sha256(fold(a)).digest(), dtype=np.uint8)


def load(path=GOLDEN_FILE):
    """{`<case>.<output>`: ("whole", array) | ("sha256", 32 bytes)}, `same_as` entries resolved."""
    with np.load(path) as z:
        index, whole, ints, sha = json.loads(str(z["index"])), z["whole"], z["whole_int"], z["sha256"]
    doc = {}
    for key, e in index.items():
        if e[0] in ("whole", "whole_int"):
            doc[key] = ("whole", (whole if e[0] == "whole" else ints)[e[1]:e[1] + int(np.prod(e[2]))].reshape(e[2]))
        elif e[0] == "sha256":
            doc[key] = ("sha256", sha[e[1]])
    for key, e in index.items():
        if e[0] == "same_as":
            doc[key] = doc[e[1]]
    return doc


def main(argv):
    if "--tree" in argv:
        sys.path.insert(0, os.path.abspath(argv[argv.index("--tree") + 1]))
    import graphsage_amd
    print("graphsage_amd from %s, library %s" % (os.path.dirname(graphsage_amd.__file__), os.environ.get("GS_LIB", "(in-tree)")))
    index, seen, whole, ints, sha = {}, {}, [], [], []
    for name in case_names():
        for key, a in run(name).items():
            a = np.ascontiguousarray(a)
            a = a.astype(np.int64) if is_int(a) else a
            assert is_int(a) or (a.dtype == np.float32 and np.isfinite(a[a != -np.inf]).all()), (name, key)
            full = "%s.%s" % (name, key)
            ident = (a.dtype.str, a.shape, fold(a))
            store = ints if is_int(a) else whole
            if ident in seen:
                index[full] = ["same_as", seen[ident]]
            elif a.nbytes <= WHOLE_BYTES:
                index[full] = ["whole_int" if is_int(a) else "whole", sum(w.size for w in store), list(a.shape)]
                store.append(a.reshape(-1))
            else:
                index[full] = ["sha256", len(sha)]
                sha.append(digest(a))
            seen.setdefault(ident, full)
        print("%-16s recorded" % name, flush=True)
    target = os.environ.get("INFER_GOLDEN_OUT", GOLDEN_FILE)
    np.savez_compressed(target, index=np.array(json.dumps(index)), whole=np.concatenate(whole), whole_int=np.concatenate(ints),
                        sha256=np.stack(sha))
    print("wrote %s (%d bytes, %d outputs)" % (target, os.path.getsize(target), len(index)))


if __name__ == "__main__":
    main(sys.argv[1:])
