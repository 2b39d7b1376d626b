"""MI355X-native embedding recommender: the hot path of Dyrutter/anime_recommendations
(neural_network / similar_anime / similar_users / model_recs) on hand-written gfx950 kernels.

Importing the package does not touch the GPU; the kernels live in libanirec.so
(built by ``anime_recommendations_amd.build``) and every op raises if it is missing.

The package leaves the runtime's hardware-queue count alone: GPUs are shared, and every process may open only as many
hardware queues as the machine allows.  Streams share a process's queues, so two chains of one cosine top-k job can
land on the same queue and serialise (350 k x 350 k top-100: 28.0 ms instead of 24.9).
"""

__version__ = "0.1.0"
