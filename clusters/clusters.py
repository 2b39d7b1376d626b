#!/usr/bin/env python
"""clusters component — the embedding table as a whole.  Every other serving component answers a question about one
anime, one user or one list; the reference draws genre word clouds per user and has nothing to say about the table.
The model can: spherical k-means on the normalised rows (``recs.cluster_rows``) cuts the anime table
into micro-genres and the user table into taste communities, exactly and reproducibly (the same seed gives the same bits
whatever the GPU does with the rows).  Its own flag set, plus

    --cluster_table anime|user      the table to cluster (default anime)
    --n_clusters <1..4096>          clusters (default 20)
    --cluster_iters <1..1000>       Lloyd iterations at most (default 50)
    --cluster_seed <int >= 0>       seed of the initial centroids, rows drawn from the table (default 0)
    --cluster_top <int >= 1>        members listed per cluster, nearest the centroid first (default 10)
    --cluster_query <name or id>    an anime name or id / a user id whose cluster is logged (default none)

Writes ``<table>_<clusters_fn>`` (one row per cluster: size, mean similarity, nearest members, leading genres) and
``<table>_assignments_<clusters_fn>`` (id, cluster, similarity of every row); the artifacts' metadata carries the
flags, the iterations run, whether the fit converged and the query's cluster."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from anime_recommendations_amd import _lib, artifacts, cli, components as C  # noqa: E402

STR_FLAGS = ["main_df", "main_df_type", "project_name", "anime_df", "anime_df_type", "model", "model_type",
             "clusters_fn", "clusters_type"]
BOOL_FLAGS = ["save_clusters"]
OPTIONAL_FLAGS = {"cluster_table": "anime", "n_clusters": 20, "cluster_iters": 50, "cluster_seed": 0,
                  "cluster_top": 10, "cluster_query": None}

logger = C.setup_logging("clusters")


def _int_in(v, lo, hi, what):
    try:
        n = int(str(v).strip())
    except ValueError:
        n = None
    if n is None or n < lo or (hi is not None and n > hi):
        raise ValueError("%r is not %s" % (v, what))
    return n


def cluster_table(v):
    s = str(v).strip().lower()
    if s not in C.CLUSTER_TABLES:
        raise ValueError("%r is not one of %s" % (v, ", ".join(C.CLUSTER_TABLES)))
    return s


def n_clusters(v):
    return _int_in(v, 1, _lib.KMEANS_MAX_K, "an integer in 1 .. %d" % _lib.KMEANS_MAX_K)


def cluster_iters(v):
    return _int_in(v, 1, _lib.KMEANS_MAX_ITER, "an integer in 1 .. %d" % _lib.KMEANS_MAX_ITER)


def cluster_seed(v):
    return _int_in(v, 0, None, "an integer >= 0")


def cluster_top(v):
    return _int_in(v, 1, None, "an integer >= 1")


def cluster_query(v):
    s = str(v).strip()
    return None if s.lower() in ("", "none") else s


def make_parser():
    p = C.make_parser("Cluster an embedding table of the ranking model: taste communities, micro-genres",
                      STR_FLAGS, BOOL_FLAGS)
    p.add_argument("--cluster_table", type=cluster_table, default=OPTIONAL_FLAGS["cluster_table"])
    p.add_argument("--n_clusters", type=n_clusters, default=OPTIONAL_FLAGS["n_clusters"])
    p.add_argument("--cluster_iters", type=cluster_iters, default=OPTIONAL_FLAGS["cluster_iters"])
    p.add_argument("--cluster_seed", type=cluster_seed, default=OPTIONAL_FLAGS["cluster_seed"])
    p.add_argument("--cluster_top", type=cluster_top, default=OPTIONAL_FLAGS["cluster_top"])
    p.add_argument("--cluster_query", type=cluster_query, default=OPTIONAL_FLAGS["cluster_query"])
    return p


def go(args):
    import numpy as np
    import pandas as pd
    from anime_recommendations_amd import recs, weights_io
    df = pd.read_parquet(artifacts.use_artifact(args.main_df, args.main_df_type))
    anime_df = C.load_anime_df(artifacts.use_artifact(args.anime_df, args.anime_df_type))
    model = weights_io.load_model(artifacts.use_artifact(args.model, args.model_type))
    user_ids, anime_ids = C.index_tables(model, df)
    table = args.cluster_table
    rows, ids = (model["A"], anime_ids) if table == "anime" else (model["U"], user_ids)
    query_row = None
    if args.cluster_query is not None:          # a query that names nothing fails before the fit
        query_row = C.cluster_query_row(table, args.cluster_query, user_ids, anime_ids, anime_df)
    logger.info("Clustering the %s table (%d rows) into %d clusters, seed %d, at most %d iterations", table, len(ids),
                args.n_clusters, args.cluster_seed, args.cluster_iters)
    fit = recs.cluster_rows(np.asarray(rows, np.float32), args.n_clusters, seed=args.cluster_seed,
                            max_iter=args.cluster_iters, normalised=False)
    logger.info("%d iterations, %s", fit["iters"], "converged" if fit["converged"] else "not converged")
    meta = C.metadata_by_index(anime_ids, anime_df)
    fav = C.favourite_bits(df, user_ids, anime_ids, C.CLUSTER_PERCENTILE) if table == "user" else None
    frame = C.clusters_frame(fit, table, ids, meta, top=args.cluster_top, fav_bits=fav)
    assignments = C.cluster_assignments_frame(fit, table, ids)
    metadata = {"cluster_table": table, "n_clusters": args.n_clusters, "cluster_iters": args.cluster_iters,
                "cluster_seed": args.cluster_seed, "cluster_top": args.cluster_top, "iterations": fit["iters"],
                "converged": bool(fit["converged"]), "cluster_query": args.cluster_query, "query_cluster": None}
    if query_row is not None:
        metadata["query_cluster"] = int(assignments["cluster"].iloc[query_row])
        logger.info("%s %s lies in cluster %d (similarity %.4f)", table, args.cluster_query, metadata["query_cluster"],
                    float(assignments["similarity"].iloc[query_row]))
    fn, afn = table + "_" + args.clusters_fn, table + "_assignments_" + args.clusters_fn
    frame.to_csv(fn, index=False)
    assignments.to_csv(afn, index=False)
    artifacts.log_artifact(fn, fn, args.clusters_type, "Clusters of the %s embedding table" % table,
                           metadata=dict(metadata, Filename=fn))
    artifacts.log_artifact(afn, afn, args.clusters_type, "Cluster of every row of the %s embedding table" % table,
                           metadata=dict(metadata, Filename=afn))
    if not args.save_clusters:
        os.remove(fn)
        os.remove(afn)
    return frame, assignments


if __name__ == "__main__":
    cli.run("clusters", logger, go, make_parser())
