/*
 * mrk.h — C ABI of libmrk_hip.so, the MI355X-native /rank hot path for Metarank.
 *
 * This is the drop-in boundary.  The Scala host keeps its HTTP API,
 * event schema, feature registry and persistence; it binds these entry points through
 * JNA / Panama and nothing else.  Plain C: opaque handles,
 * caller-owned buffers, no exceptions, no C++/torch types in any signature.
 *
 * Every function returns MRK_OK (0) on success and a negative mrk_status on failure;
 * mrk_last_error() returns a thread-local human readable message for the last failure
 * on the calling thread.  Handles are thread-safe: many request threads may call
 * mrk_model_predict_f64 / mrk_rank on the same handles concurrently while a feedback
 * thread calls mrk_store_put_* (reference threading model: cats-effect compute pool,
 * src/main/scala/ai/metarank/ml/rank/LambdaMARTRanker.scala:348 and
 * src/main/scala/ai/metarank/fstore/cache/CachedModelStore.scala:39-42).
 *
 * Reference interfaces replaced (all paths relative to the reference repo root,
 * M = src/main/scala/ai/metarank):
 *
 *   mrk_model_load*            <- LightGBMBooster(bytes) / XGBoostBooster(bytes)
 *                                 M/ml/rank/LambdaMARTRanker.scala:228-232 and the
 *                                 bitstream reader :192-236
 *   mrk_model_predict_f64      <- ltrlib Booster.predictMat(values, rows, cols)
 *                                 M/ml/rank/LambdaMARTRanker.scala:348
 *   mrk_model_free             <- Booster.close()/isClosed() :361-365
 *   mrk_config_load_json       <- FeatureMapping.fromFeatureSchema + makeDatasetDescriptor
 *                                 M/FeatureMapping.scala:56-99
 *   mrk_store_put_*            <- KVStore[Key,FeatureValue].put  M/fstore/Persistence.scala:85-89
 *                                 fed by FeatureValueSink.write   M/flow/FeatureValueSink.scala:10-14
 *   mrk_rank, mrk_rank_binary, <- Ranker.rerank = makeQuery + predict + sortBy(-score)
 *   mrk_batch_*                   M/ml/Ranker.scala:27-83,97-106
 *   mrk_model_weights          <- ltrlib Booster.weights()  M/ml/rank/LambdaMARTRanker.scala:391-406
 *   mrk_init(devices, n)       <- HipConfig(inner, devices: List[Int]) next to LightGBMConfig / XGBoostConfig
 *                                 M/config/BoosterConfig.scala:96-104 (SURVEY.md 8b touch point 1): one context per device,
 *                                 all inside the one host process (M/main/command/Serve.scala:72-128)
 *   mrk_index_*                <- KnnIndexWriter.write / KnnIndexReader.lookup  M/ml/recommend/embedding/HnswJavaIndex.scala:23-87,
 *                                 EmbeddingSimilarityModel.predict  M/ml/recommend/MFRecommender.scala:66-80
 *   mrk_trending_*             <- TrendingPredictor.fit / load, TrendingModel.predict / save
 *                                 M/ml/recommend/TrendingRecommender.scala:39-133
 *   mrk_als_*                  <- MFPredictor.fit + ALSRecImpl.train  M/ml/recommend/MFRecommender.scala:26-63,
 *                                 M/ml/recommend/mf/ALSRecImpl.scala:18-81
 *   mrk_encoder_*              <- OnnxSession / OnnxBiEncoder / OnnxCrossEncoder  M/ml/onnx/sbert/ (OnnxSession, OnnxBiEncoder, OnnxCrossEncoder .scala)
 *
 * ABI 8 (round 5): mrk_init creates n contexts; mrk_device_count; mrk_comm_init_local; mrk_model_inspect; mrk_serve_stats takes
 * the length of its output array; mrk_store_put_binary_at / mrk_store_expire; mrk_encoder_load is f32 (MRK_ENCODER_AUTO = F32).
 * ABI 9 (round 6): mrk_model_weights / mrk_model_inspect_weights (Booster.weights()), mrk_abi_layout.  Same ABI, new behaviour:
 * the serving queue's slots are launched in gangs (64 slots on 8 streams) and mrk_rank answers through a started queue.
 * Still ABI 9, new symbols only: mrk_index_* (the similar-items index of /recommend).
 * Still ABI 9, new symbols only: mrk_trending_* (the trending recommender of /recommend).
 * Still ABI 9, new symbols only: mrk_index_build_texts (the semantic recommender's fit), mrk_index_vectors.
 * Still ABI 9, new symbols only: mrk_als_* (the similar-items recommender's fit: eALS factors on the device).
 * Still ABI 9, no new symbol and no struct change: mrk_train_* takes the config key "backend" ("xgboost": the level-wise fit that
 * returns XGBoost JSON) and its keys lambda, gamma, min_child_weight; without the key a fit gives the bytes it gave before.
 * Still ABI 9, new symbols only: mrk_train_append_device, mrk_train_seal (the trainer's matrix from device memory, its bins found on
 * the device) and mrk_train_bounds.
 */
#ifndef MRK_H
#define MRK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MRK_ABI_VERSION 9

typedef enum mrk_status {
  MRK_OK = 0,
  MRK_ERR_INVALID_ARG = -1,   /* null handle, bad sizes, unknown enum                    */
  MRK_ERR_PARSE = -2,         /* model / config bytes could not be parsed                 */
  MRK_ERR_DEVICE = -3,        /* HIP runtime failure (message carries hipGetErrorString)  */
  MRK_ERR_DIM_MISMATCH = -4,  /* IllegalStateException "dim mismatch" M/model/ItemValue.scala:47,56,60 */
  MRK_ERR_ARITHMETIC = -5,    /* java.lang.ArithmeticException: / by zero in the normalised rate,
                                 M/feature/RateFeature.scala:346-348 (global top counter == 0)  */
  MRK_ERR_UNSUPPORTED = -6,   /* valid input the device path does not implement (yet)     */
  MRK_ERR_NOT_FOUND = -7,     /* unknown model / feature name                             */
  MRK_ERR_FEATURE_MISMATCH = -8 /* "booster trained with X features, but config defines Y"
                                 M/ml/rank/LambdaMARTRanker.scala:208-213                   */
} mrk_status;

typedef struct mrk_ctx mrk_ctx;       /* one per process per device set           */
typedef struct mrk_model mrk_model;   /* one per loaded booster (ref-counted)     */
typedef struct mrk_batch mrk_batch;   /* a prepared, device-resident request batch */

/* ---------------------------------------------------------------- lifecycle */

int mrk_abi_version(void);
/* identifies the library's SOURCES (hex digest over csrc/ and this header, fixed when the library is built) */
const char *mrk_build_id(void);
const char *mrk_last_error(void);
/* Layout of every struct that crosses the boundary by value or by pointer, as THIS library was compiled: what a JNA
 * @FieldOrder Structure checks at start-up instead of trusting its own copy of this header.  Writes up to
 * `cap` int32 into out (nullable) and returns how many there are:
 *   [0] MRK_ABI_VERSION
 *   [1..8]   mrk_field:      sizeof, then offsetof name, type, n, num, str, strs, nums
 *   [9..19]  mrk_request:    sizeof, then offsetof id, timestamp_ms, user, session, fields, n_fields, n_items, item_ids,
 *                            item_field_offsets, item_fields
 *   [20..32] mrk_model_info: sizeof, then offsetof backend, n_trees, max_depth, n_features, is_f64, n_categorical, n_nodes,
 *                            n_leaves, device_bytes, base_score, bitvector, tile_columns */
int mrk_abi_layout(int32_t *out, int cap);

/* One context per listed HIP ordinal, all in the calling process: out[0 .. n_devices) (HipConfig(inner, devices: List[Int]),
 * SURVEY 8b touch point 1; the reference's host is ONE JVM, M/main/command/Serve.scala:72-128).  A context owns its streams,
 * its replica of the feature store, its models and batches; every entry point selects its context's device for the calling
 * thread, nothing is per-process, so contexts are driven concurrently from different host threads (one thread per context
 * for the serving loop; puts may come from any thread).  The same ordinal may appear more than once (independent contexts
 * sharing a GPU).  n_devices = 1 is the single-device case.  On failure nothing is created.  Contexts of one process are
 * joined into an RCCL communicator by mrk_comm_init_local, contexts of different processes by mrk_comm_init. */
int mrk_init(const int *device_ids, int n_devices, mrk_ctx **out);
int mrk_device_count(void); /* HIP devices visible to this process (0: none / no driver): what HipConfig.devices is validated against */
void mrk_shutdown(mrk_ctx *ctx);

/* ------------------------------------------------- model (replaces Booster) */

enum { MRK_BACKEND_LIGHTGBM = 0, MRK_BACKEND_XGBOOST = 1 }; /* = boosterTag, LambdaMARTRanker.scala:229-230 */

/* Inner booster bytes: LightGBM model string, or XGBoost JSON / UBJSON.  Bytes are copied. */
int mrk_model_load(mrk_ctx *ctx, int backend, const uint8_t *bytes, size_t len, mrk_model **out);

/* Metarank model container (bitstream v2/v3, LambdaMARTRanker.scala:367-389).
 * If feature_names != NULL the stored list must equal it in order, else MRK_ERR_FEATURE_MISMATCH. */
int mrk_model_load_container(mrk_ctx *ctx, const uint8_t *blob, size_t len,
                             const char *const *feature_names, int n_features, mrk_model **out);

/* == predictMat: rowmajor is rows*cols f64 (host memory), out_scores is rows f64 (host memory). */
int mrk_model_predict_f64(mrk_model *model, const double *rowmajor, int rows, int cols,
                          double *out_scores);
/* Same with all three buffers already in device memory of ctx's device (no copies, async on the
 * context stream; call mrk_sync before reading). */
int mrk_model_predict_device(mrk_model *model, const double *d_rowmajor, int rows, int cols,
                             double *d_out_scores);

typedef struct mrk_model_info {
  int32_t backend;       /* MRK_BACKEND_*                                   */
  int32_t n_trees;
  int32_t max_depth;     /* longest root->leaf path in node visits          */
  int32_t n_features;    /* max_feature_idx + 1 / num_feature               */
  int32_t is_f64;        /* 1: LightGBM f64 arithmetic, 0: XGBoost f32       */
  int32_t n_categorical; /* number of categorical split nodes               */
  int64_t n_nodes;       /* internal nodes                                  */
  int64_t n_leaves;
  int64_t device_bytes;  /* packed forest bytes resident in HBM             */
  double base_score;     /* XGBoost base margin (0.0 for LightGBM)          */
  int32_t bitvector;     /* 1: every tree has <= 16 leaves, the bit-vector scorer applies; 0: tree-walk scorer */
  int32_t tile_columns;  /* bitvector: columns ("views") of the scorer's binned tile */
} mrk_model_info;
int mrk_model_get_info(mrk_model *model, mrk_model_info *out);
/* Host-only (no context, no device): reads, validates and packs a booster exactly as mrk_model_load would and reports what it
 * found (device_bytes = what the load would place in HBM) - MRK_ERR_PARSE for malformed bytes, MRK_ERR_UNSUPPORTED for a
 * well-formed model the scorer does not implement (dart, multi-output, vector leaves, num_parallel_tree > 1, a non-identity
 * objective, linear trees, random-forest averaging).  What a host calls when it validates a config. */
int mrk_model_inspect(int backend, const uint8_t *bytes, size_t len, mrk_model_info *out);

/* == ltrlib Booster.weights(): Array[Double], one entry per matrix column (reference call site
 * M/ml/rank/LambdaMARTRanker.scala:391-406: `w(offset)` / `w.slice(offset, offset + size)` per descriptor feature).  out[0 .. n_cols):
 * n_cols = the DatasetDescriptor's dimension; columns past the model's n_features get 0.0; n_cols < n_features is
 * MRK_ERR_DIM_MISMATCH (the JVM would throw IndexOutOfBounds).  Computed on the host from the parsed booster with the owning
 * library's own arithmetic:
 *   LightGBM  (LGBM_BoosterFeatureImportance, GBDT::FeatureImportance, num_iteration 0): SPLIT = number of splits on the feature
 *             with split_gain > 0; GAIN = TOTAL_GAIN = sum of those float gains accumulated in double, tree order then node order.
 *   XGBoost   (Booster.getScore, GBTree::FeatureScore): SPLIT = "weight" = number of splits; TOTAL_GAIN = "total_gain" = sum of
 *             loss_chg accumulated in float; GAIN = "gain" = total_gain / weight in float; a feature never split on is absent
 *             from the JVM's map - 0.0 here.
 * ASSUMPTION (ltrlib 0.2.6 is not in the reference tree): its LightGBMBooster.weights() asks lightgbm4j for
 * FeatureImportanceType.GAIN and its XGBoostBooster.weights() fills an array from getScore("", "gain"): a HipBooster passes
 * MRK_IMPORTANCE_GAIN for both.  Unverifiable here; if ltrlib uses another type the binding changes one constant.  A model file
 * without split gains (no `split_gain=` / "loss_changes") answers GAIN / TOTAL_GAIN with MRK_ERR_UNSUPPORTED. */
enum { MRK_IMPORTANCE_SPLIT = 0, MRK_IMPORTANCE_GAIN = 1, MRK_IMPORTANCE_TOTAL_GAIN = 2 };
int mrk_model_weights(mrk_model *model, int importance_type, double *out, int n_cols);
/* the same host-only, from booster bytes (no context, no device): config validation, CPU tests */
int mrk_model_inspect_weights(int backend, const uint8_t *bytes, size_t len, int importance_type, double *out, int n_cols);

void mrk_model_retain(mrk_model *model);
void mrk_model_free(mrk_model *model); /* drops one reference; idempotent at zero (close()/isClosed()) */

/* ------------------------------------ feature schema (FeatureMapping mirror) */

/* json: {"features":[<Metarank feature schemas>], "models": {"<name>": {"type":"lambdamart",
 * "features":[...]}}} i.e. the `features:` and `models:` sections of Metarank's config.yml
 * rendered as JSON (the Scala host has circe encoders for every schema).  Builds the feature
 * registry, the device store layout and, per lambdamart model, the DatasetDescriptor
 * (column order = models.<name>.features order, M/FeatureMapping.scala:66-72,89-99). */
int mrk_config_load_json(mrk_ctx *ctx, const char *json, size_t len);

/* number of matrix columns (DatasetDescriptor.dim) for a configured model, <0 on error */
int mrk_model_dim(mrk_ctx *ctx, const char *model_name);
/* Host-only (no device, no context): what the library builds the first time a model of this config is ranked - the
 * assembly kernel specialised for the model's feature list (the reference fixes that list per model when the config is
 * loaded, M/FeatureMapping.scala:56-99; here it becomes compile-time constants of the kernel).  f64: scorer precision the
 * kernel bins for (1 LightGBM, 0 XGBoost).  what = 0: the HIP source handed to hiprtc; what = 1: the gfx950 code object -
 * of all specialised kernels; `what | (k << 8)`, k = 1..4: of the one kernel the library would compile by itself (1 the
 * workgroup-per-request kernel of full batches, 2 its op-split / sliced form, 3 its f64-matrix form, 4 the item-parallel kernel).
 * The single-kernel index stops at k = 9 (the kernels mrk_config_precompile's bits 0 .. 8 name): the one-launch kernel and the
 * persistent workgroup of forests scored by the tree walk (precompile bits 9 / 10) are part of the all-kernels form only.
 * MRK_ERR_INVALID_ARG with *needed set (for what = 1: to an upper bound) when `out` is NULL or `cap` too small; *needed is
 * the exact size on success. */
int mrk_config_specialize(const char *json, size_t len, const char *model_name, int f64, int what, uint8_t *out, size_t cap,
                          size_t *needed);

/* Host-only: writes into directory `dir` the gfx950 code object of every specialised kernel in `kernel_mask` (bit k: 0 the
 * workgroup-per-request kernel, 1 its op-split / sliced form, 2 the f64-matrix form, 3 the item-parallel kernel, 4 the
 * one-launch kernel of mrk_rank, 5 the persistent workgroup of the serving queue, 6 no kernel any more - the bit is accepted
 * and compiles nothing, so that masks written for earlier versions keep working -, 7 the stand-alone pre-pass of requests too
 * large for one workgroup, 9 / 10 the one-launch kernel / the persistent workgroup of
 * forests scored by the tree walk) for this config's model - what a
 * deployment ships next to libmrk_hip.so (directory `jit_cache`) so that no process ever compiles: the library looks
 * there, then in the user's cache ($MRK_JIT_CACHE_DIR, ~/.cache/mrk_jit), and only then compiles - in the BACKGROUND,
 * ranking with the kernel that interprets the program meanwhile (MRK_RANK_JIT: 0 never specialise, 1 wait for the compiler,
 * require, async, auto = this default).  out_compiled (nullable): how many were not there yet. */
int mrk_config_precompile(const char *json, size_t len, const char *model_name, int f64, unsigned kernel_mask, const char *dir,
                          int *out_compiled);
/* The kernels that write the scorer's binned tile are keyed by the FOREST too - by its view signature: per matrix column
 * which tile columns it fills (NaN / zero / categorical routing kinds) and how many 128-entry chunks its threshold table
 * takes; not the thresholds, not the trees - and hold it as compile-time constants (no descriptor loads, no view loops).
 * Retraining on the same features usually keeps the signature, hence the kernels.  The two entry points above know the
 * config only: they build the signature-less kernels, which serve any model of the program while its own kernels compile.
 * These two do the same for one serialised booster (backend / bytes as for mrk_model_load; the precision follows from the
 * backend): what a deployment runs when it ships a model.  Host-only. */
int mrk_config_specialize_for_model(const char *json, size_t len, const char *model_name, int backend, const uint8_t *model_bytes,
                                    size_t model_len, int what, uint8_t *out, size_t cap, size_t *needed);
int mrk_config_precompile_for_model(const char *json, size_t len, const char *model_name, int backend, const uint8_t *model_bytes,
                                    size_t model_len, unsigned kernel_mask, const char *dir, int *out_compiled);
/* Which specialised kernels of this model are loaded, as text: one line "<kernel name> <key> program|program+forest" each;
 * <key> = the stem of the kernel's cache file (hash and size of its translation unit, compiler version).  With mrk_build_id
 * this is what a measurement records to say WHICH code it measured (bench.py `provenance`).  MRK_ERR_INVALID_ARG with *needed
 * set (bytes incl. the terminating 0) when `out` is NULL or `cap` too small. */
int mrk_config_kernel_keys(mrk_ctx *ctx, const char *model_name, char *out, size_t cap, size_t *needed);
/* Serve.maybeWarmup for the kernels: waits until the background compiles of this model's kernels that are under way have
 * finished (the next launch uses them).  A host calls it before it opens its port; nothing on the request path waits. */
int mrk_config_warmup(mrk_ctx *ctx, const char *model_name);

/* ------------------------- feature store (KVStore[Key, FeatureValue] mirror) */

/* `key` is Key.encode (M/model/Key.scala:9): "<ScopeCodec.encode(scope)>/<feature name>", e.g.
 * "item=42/popularity", "global/ctr_click_norm", "field=genre:drama/ctr_genre_click",
 * "session=s1/profile_interactions", "irf=query:socks:p1/ctr_click".
 * Each put replaces the previous value of that key (KVStore.put semantics).  Puts are staged on
 * the host and become visible to mrk_rank calls that start after mrk_store_flush returns
 * (mrk_rank / mrk_batch_prepare flush implicitly). */
int mrk_store_put_double(mrk_ctx *ctx, const char *key, double v);               /* ScalarValue(SDouble)      */
int mrk_store_put_bool(mrk_ctx *ctx, const char *key, int v);                    /* ScalarValue(SBoolean)     */
int mrk_store_put_string(mrk_ctx *ctx, const char *key, const char *v);          /* ScalarValue(SString)      */
int mrk_store_put_string_list(mrk_ctx *ctx, const char *key, const char *const *v, int n); /* SStringList    */
int mrk_store_put_double_list(mrk_ctx *ctx, const char *key, const double *v, int n);      /* SDoubleList    */
int mrk_store_put_counter(mrk_ctx *ctx, const char *key, int64_t v);             /* CounterValue             */
int mrk_store_put_periodic(mrk_ctx *ctx, const char *key, const int64_t *values, int n); /* PeriodicCounterValue.values(i).value */
int mrk_store_put_bounded_list(mrk_ctx *ctx, const char *key, const char *const *values, int n); /* BoundedListValue of SString */
int mrk_store_delete(mrk_ctx *ctx, const char *key);

/* Bulk load from the reference's binary wire format: `bytes` is any concatenation of
 * FeatureValueCodec records (M/fstore/codec/impl/FeatureValueCodec.scala:40-168, tags 0-13) - what the
 * Redis / RocksDB / MapDB `values` store holds per key.  Every record is applied like the matching
 * mrk_store_put_* (NumStats / Map / Frequency values are parsed and ignored: /rank does not read them).
 * out_records (nullable) receives the number of records decoded. */
int mrk_store_put_binary(mrk_ctx *ctx, const uint8_t *bytes, size_t len, int *out_records);
/* FeatureValue.expire (FeatureValueCodec.scala:42-48,75: every record carries its feature's ttl; the Redis store drops a key that
 * long after its LAST write, RedisKVStore.scala:40 - the other engines never do).  mrk_store_put_binary ignores it.  A host whose
 * system of record expires keys uses mrk_store_put_binary_at instead: the same load, and every applied record is remembered
 * with deadline = now_ms + expire (now_ms: the host's clock, Timestamp.now; pre-ttl encodings count as 90 days); a later write
 * of the same key through ANY put replaces or clears its deadline.  mrk_store_expire(ctx, now_ms, &n) - called from a timer -
 * deletes the values whose deadline has passed (exactly mrk_store_delete; the next flush uploads the change).  Host memory:
 * about 40 bytes per live deadline; nothing when the _at form is never used. */
int mrk_store_put_binary_at(mrk_ctx *ctx, const uint8_t *bytes, size_t len, int64_t now_ms, int *out_records);
int mrk_store_expire(mrk_ctx *ctx, int64_t now_ms, int64_t *out_expired);

/* Write path: instead of a refreshed FeatureValue the host may forward the raw Writes of
 * FeatureValueFlow.commitWrite (M/flow/FeatureValueFlow.scala:44-62); the FeatureValue the read path needs is
 * then derived by the library - always fresh, no `refresh` interval.
 *   mrk_store_increment_periodic  Write.PeriodicIncrement(key, ts, inc): added to the key's bucket ring in HBM
 *                                 (bucket = ts.toStartOfPeriod(bucket)); the window sums of
 *                                 PeriodicCounterFeature.fromMap (M/model/Feature.scala:142-161) are recomputed on
 *                                 the device at the next flush.  A key is fed either by these or by
 *                                 mrk_store_put_periodic, not both (the ring wins).
 *   mrk_store_increment           Write.Increment(key, ts, inc) -> CounterValue
 *   mrk_store_append              Write.Append(key, SString(value), ts) -> BoundedListValue, bounded by the
 *                                 feature's count / duration (M/fstore/memory/MemBoundedList.scala:18-37) */
int mrk_store_increment_periodic(mrk_ctx *ctx, const char *key, int64_t ts_ms, int64_t inc);
/* n PeriodicIncrements in one call (one event usually produces several: item, field-scoped, global keys) */
int mrk_store_increment_periodic_batch(mrk_ctx *ctx, const char *const *keys, const int64_t *ts_ms, const int64_t *inc, int n);
int mrk_store_increment(mrk_ctx *ctx, const char *key, int64_t inc);
int mrk_store_append(mrk_ctx *ctx, const char *key, const char *value, int64_t ts_ms);
int mrk_store_flush(mrk_ctx *ctx);

/* ---------------------------------------------------------------- requests */

enum {
  MRK_FIELD_STRING = 0,      /* Field.StringField     */
  MRK_FIELD_NUMBER = 1,      /* Field.NumberField     */
  MRK_FIELD_BOOL = 2,        /* Field.BooleanField    */
  MRK_FIELD_STRING_LIST = 3, /* Field.StringListField */
  MRK_FIELD_NUMBER_LIST = 4  /* Field.NumberListField */
};

typedef struct mrk_field {
  const char *name;
  int32_t type;               /* MRK_FIELD_*                                  */
  int32_t n;                  /* list length for the *_LIST types              */
  double num;                 /* NUMBER / BOOL (0|1)                           */
  const char *str;            /* STRING                                        */
  const char *const *strs;    /* STRING_LIST                                   */
  const double *nums;         /* NUMBER_LIST                                   */
} mrk_field;

/* RankingEvent (M/model/Event.scala) restricted to what the hot path reads. */
typedef struct mrk_request {
  const char *id;             /* RankingEvent.id                                */
  int64_t timestamp_ms;       /* RankingEvent.timestamp.ts                      */
  const char *user;           /* nullable                                       */
  const char *session;        /* nullable                                       */
  const mrk_field *fields;    /* ranking-level fields                           */
  int32_t n_fields;
  int32_t n_items;
  const char *const *item_ids;        /* n_items item ids, request order        */
  const int32_t *item_field_offsets;  /* nullable; CSR n_items+1 offsets into item_fields */
  const mrk_field *item_fields;       /* per-item fields (relevancy, overrides) */
} mrk_request;

/* Ranker.rerank for one request.  out_scores[n_items]: score of item i (request order);
 * out_order[n_items]: indices into the request in response order (stable sort by -score with
 * java.lang.Double.compare semantics); out_matrix: nullable, n_items*dim row-major f64 = the
 * ClickthroughQuery matrix (explain / parity). */
int mrk_rank(mrk_ctx *ctx, mrk_model *model, const char *model_name, const mrk_request *req,
             double *out_scores, int32_t *out_order, double *out_matrix);

/* The same for a request in the reference's binary RankingEventFormat (M/util/RankingEventFormat.scala:12-62; the
 * encoding of the warm-up requests inside the model container, and a cheaper wire form than JSON for a host that
 * already holds the event).  `event` holds one record; out_n_items receives its item count; out_scores /
 * out_order must have room for `capacity` items (MRK_ERR_INVALID_ARG with out_n_items set if it has more). */
int mrk_rank_binary(mrk_ctx *ctx, mrk_model *model, const char *model_name, const uint8_t *event, size_t len,
                    int *out_n_items, double *out_scores, int32_t *out_order, int capacity);
/* ---- training rows: ItemValue.fromState in ValueMode.OfflineTraining ------------------------------------------------
 * The reference calls ItemValue.fromState from two places: Ranker.makeQuery (OnlineInference, the model's features: mrk_rank)
 * and TrainBuffer.handleRanking (M/flow/TrainBuffer.scala:51-71: OfflineTraining, EVERY feature of the mapping, once per
 * ranking event that comes through /feedback or `import`; its result is ClickthroughValues.values, the row a later training
 * reads).  mrk_values answers the second call.
 *   model_name  NULL: the MAPPING program - every feature of `features:`, in the order fromState emits values
 *               (M/model/ItemValue.scala:32-69): the RankingFeatures (local_time, ua, referer) in `features:` order, then the
 *               ItemFeatures in `features:` order.  ua / referer / random / field_match without "match": "device" are
 *               "__ext:<name>" inputs with their "dim", as in model programs.  A model's name: that model's columns
 *               (DatasetDescriptor order, as mrk_rank's matrix).
 *   mode        0 OnlineInference, 1 OfflineTraining.  The one feature that reads it is `position`
 *               (M/feature/PositionFeature.scala:32-33): online the configured constant, offline the candidate's index in its
 *               request (0, 1, 2, ...).  mode 0 with a model's name is mrk_rank(model = NULL, out_matrix)'s matrix.
 *   out_matrix  n_items x mrk_values_dim() f64, row-major.  A CategoryValue column carries the category's INDEX (what
 *               ClickthroughQuery.collectFeatureValues reads); CategoryValue.cat is not returned - the host has it as
 *               values[index - 1] of the feature's schema ("nil" for 0).
 * Statuses are mrk_rank's (MRK_ERR_DIM_MISMATCH, MRK_ERR_ARITHMETIC of the normalised rate, ...).  Small requests take ONE
 * kernel launch whose stores go straight into pinned host memory (no forest, no ordering, no copy command); requests of
 * more than a workgroup's lanes, requests with per-item overrides and programs with a request-normalised column take the
 * assembly launches and a copy.  Callers of one context are served one at a time; hosts that batch use mrk_batch_load_values.
 * mrk_values_binary: the same for a request in the reference's binary RankingEventFormat (mrk_rank_binary's decoder);
 * out_matrix must have room for `capacity` items.
 * mrk_values_dim: columns of a row (model_name NULL: of the mapping program), <0 on error.
 * mrk_values_columns: text, one line per feature in column order: "<name>\t<first column>\t<dim>\t<single|vector|category>\n"
 * - the MValue the reference's feature emits (SingleValue / VectorValue / CategoryValue(index)); NUL-terminated; sizing as
 * mrk_config_kernel_keys.
 * mrk_batch_load_values: mrk_batch_load for a values program; mrk_batch_run(batch, NULL) then assembles the rows (scores are
 * 0.0 and every request keeps its own order, as NoopRanker's), mrk_batch_fetch(out_matrix) / mrk_batch_status read them.
 * mrk_config_specialize_values: mrk_config_specialize (f64 = 1) for a values program; kernel 12 (what = 12 << 8 | form) is the
 * one-launch values kernel.  An offline program with a `position` feature holds the item-index op (kind 15); online ones and
 * programs without `position` do not, and their kernels are the ones mrk_rank runs. */
int mrk_values(mrk_ctx *ctx, const char *model_name, int mode, const mrk_request *req, double *out_matrix);
int mrk_values_binary(mrk_ctx *ctx, const char *model_name, int mode, const uint8_t *event, size_t len, int *out_n_items,
                      double *out_matrix, int capacity);
int mrk_values_dim(mrk_ctx *ctx, const char *model_name);
int mrk_values_columns(mrk_ctx *ctx, const char *model_name, char *out, size_t cap, size_t *needed);
/* host-only (no device, no context), as mrk_config_specialize: the same text for a config that is not loaded anywhere */
int mrk_config_values_columns(const char *json, size_t len, const char *model_name, char *out, size_t cap, size_t *needed);
int mrk_config_specialize_values(const char *json, size_t len, const char *model_name, int mode, int what, uint8_t *out,
                                 size_t cap, size_t *needed);
/* Warm-up (Serve.maybeWarmup, M/main/command/Serve.scala:130-150): a model loaded with mrk_model_load_container keeps
 * the container's warm-up requests; mrk_model_warmup ranks each of them once (results discarded) and returns the
 * number replayed through out_replayed. */
int mrk_model_warmup(mrk_ctx *ctx, mrk_model *model, const char *model_name, int *out_replayed);

/* Batched form: resolve n_req requests once into a device-resident batch, then run it any number
 * of times (the benchmark's device-only timed region is mrk_batch_run only). */
int mrk_batch_prepare(mrk_ctx *ctx, const char *model_name, const mrk_request *reqs, int n_req,
                      mrk_batch **out);

/* ---- the serving loop: reusable batches, flat item ids, results in pinned memory ----------------------------------
 * What a host that decodes `ranking` events off the wire has in its hands is the UTF-8 bytes of the item ids, not an
 * array of C strings - and the first hop of the read path (FeatureValueLoader.fromStateBackend building one
 * Key(ItemScope(id), feature) per candidate, M/fstore/FeatureValueLoader.scala:11-25, M/model/Key.scala:7-10) is an id
 * lookup per candidate.  With flat ids that hop runs on the device: the id bytes are uploaded as they are and a kernel
 * hashes, probes the device mirror of the store's id table and compares (csrc/resolve.hip); the host does O(requests)
 * work, nothing per item.
 *
 *   mrk_batch_create   an empty batch that owns a HIP stream and grow-only buffers;
 *   mrk_batch_load     (re)fills it: waits for the batch's previous work, resolves the request-level part on the host
 *                      (user / session / ranking slots, request constants, table sizing from bounds), uploads, and - with
 *                      `ids` - enqueues the id resolution.  ids == NULL: reqs[r].item_ids are used (host lookups, exact
 *                      table sizes), exactly like mrk_batch_prepare.  With ids, reqs[r].item_ids is ignored: the ids of
 *                      request 0's items, then request 1's, ... lie back to back in ids->bytes, item i of the batch
 *                      being bytes[offsets[i], offsets[i + 1]).  Buffers obtained from mrk_host_alloc are read by the
 *                      copy engine directly; any other memory is staged through the batch's pinned buffer.
 *   mrk_batch_run      as before (asynchronous);
 *   mrk_batch_enqueue_fetch  enqueues the download of scores / order / status into the batch's pinned result buffer
 *                      behind the run (asynchronous);
 *   mrk_batch_host_outputs   waits for the batch and returns pointers INTO that pinned buffer (valid until the next
 *                      mrk_batch_load / mrk_batch_run of this batch): scores[total_items] (request order), order
 *                      [total_items] (request-local indices in response order), status[n_req] (mrk_status per request).
 * Several batches of a context may be loaded, run and fetched from different host threads at the same time; store puts
 * are serialised against them (a put never changes what a batch already in flight reads). */
typedef struct mrk_item_ids {
  const uint8_t *bytes;     /* concatenated UTF-8 ids, no terminators                  */
  const uint32_t *offsets;  /* total_items + 1 byte offsets into `bytes`, ascending    */
  size_t bytes_len;         /* size of `bytes`: offsets[total_items] must not exceed it.  Offsets come off the wire: a
                               batch whose last offset passes bytes_len is refused (MRK_ERR_INVALID_ARG); an item whose
                               offsets descend or pass bytes_len fails ITS request with MRK_ERR_INVALID_ARG (checked by
                               the id-resolution kernel, and by the host wherever it reads an id itself)            */
} mrk_item_ids;
/* LIFETIME of ids->bytes / ids->offsets: pinned buffers (mrk_host_alloc) are read by the copy engine AFTER mrk_batch_load
 * has returned - do not rewrite or free them before the next mrk_batch_sync / mrk_batch_host_outputs / mrk_batch_fetch of
 * this batch.  Pageable memory is copied before mrk_batch_load returns and may be reused at once. */
int mrk_batch_create(mrk_ctx *ctx, mrk_batch **out);
int mrk_batch_load(mrk_batch *batch, const char *model_name, const mrk_request *reqs, int n_req, const mrk_item_ids *ids);
int mrk_batch_load_values(mrk_batch *batch, const char *model_name /* NULL: the mapping program */, int mode, const mrk_request *reqs,
                          int n_req, const mrk_item_ids *ids);   /* see mrk_values */
int mrk_batch_enqueue_fetch(mrk_batch *batch);
int mrk_batch_host_outputs(mrk_batch *batch, const double **scores, const int32_t **order, const int32_t **status);
/* pinned (page-locked) host memory the device can read / write without a staging copy; NULL on failure */
void *mrk_host_alloc(size_t bytes);
void mrk_host_free(void *p);
int mrk_batch_total_items(mrk_batch *batch);
/* asynchronous on the context stream */
int mrk_batch_run(mrk_batch *batch, mrk_model *model);
/* Item-sharded execution (the reference has no counterpart - it scores a request on one
 * JVM thread): shard `shard_index` of `shard_count` assembles and scores batch items
 * [index * chunk, (index + 1) * chunk) only, chunk = mrk_batch_shard_chunk() (total / count rounded up to a
 * whole number of 128-item scorer tiles), and does NOT sort.  Request-level reductions (diversity,
 * interacted_with) are computed from the whole request on every shard; a model with a request-normalised column
 * (bi- / cross-encoder `norm`) has its whole matrix assembled and normalised on every shard - only the forest is
 * shared out.  The caller merges the score
 * slices of all shards into the device score buffer (one all-gather of chunk * count f64; the buffer
 * has room for the padded tail) and then calls mrk_batch_sort on the rank(s) that need the order. */
int mrk_batch_shard_chunk(mrk_batch *batch, int shard_count);
/* The shard arithmetic by itself - host-only, no context, no device (a host lays out its buffers with it, the CPU tests
 * of the N > 1 path check it): mrk_shard_chunk = ceil(total_items / shard_count) rounded up to whole MRK_SHARD_TILE-item
 * scorer tiles (negative mrk_status on bad arguments); mrk_shard_range = the items [lo, hi) shard `shard_index` assembles
 * and scores: [index * chunk, (index + 1) * chunk) clipped to total_items (trailing shards may be empty). */
#define MRK_SHARD_TILE 128
int64_t mrk_shard_chunk(int64_t total_items, int shard_count);
int mrk_shard_range(int64_t total_items, int shard_index, int shard_count, int64_t *lo, int64_t *hi);
int mrk_batch_run_shard(mrk_batch *batch, mrk_model *model, int shard_index, int shard_count);
int mrk_batch_sort(mrk_batch *batch);
/* A prepared batch owns a HIP stream: batches of one context may be in flight together (mrk_batch_run is
 * asynchronous), which is how consecutive batches overlap on the device - the assembly kernels wait on memory,
 * the scorer is VALU-bound.  mrk_batch_sync waits for this batch; mrk_batch_fetch / _status synchronise it too.
 * mrk_store_flush (and every put that grows a table) waits for all batches before it rewrites device memory. */
void *mrk_batch_stream(mrk_batch *batch);
int mrk_batch_sync(mrk_batch *batch);
/* device pointers of the batch outputs (valid until mrk_batch_free): scores f64[total_items],
 * order i32[total_items] (request-local indices), matrix f64[total_items*dim].
 * The f64 matrix (ClickthroughQuery's layout) is materialised on demand only: with a LightGBM /
 * XGBoost model of <= 16-leaf trees the assembled values go straight into the scorer's binned
 * tile.  Asking for d_matrix here makes every later mrk_batch_run of this batch write it;
 * mrk_batch_fetch(out_matrix != NULL) and mrk_rank(out_matrix != NULL) materialise it for that call. */
int mrk_batch_device_outputs(mrk_batch *batch, double **d_scores, int32_t **d_order, double **d_matrix);
/* copy results to host (synchronises); any pointer may be NULL */
int mrk_batch_fetch(mrk_batch *batch, double *out_scores, int32_t *out_order, double *out_matrix);
/* per-request outcome of the last run: out_status[n_req] = MRK_OK or the mrk_status the reference's
 * exception for that request maps to (e.g. MRK_ERR_ARITHMETIC); results of failed requests are undefined */
int mrk_batch_status(mrk_batch *batch, int32_t *out_status);
void mrk_batch_free(mrk_batch *batch);

/* ---- the serving queue ---------------------------------------------------------------------------
 * Replaces the request loop around Ranker.rerank - main/command/Serve.scala:130-150 (warm-up, then the port opens) and
 * api/routes/RankApi.scala:25-41 (one rerank per request thread).  mrk_serve_start compiles what the model needs (the
 * warm-up: no request ever waits for a compiler) and prepares n_slots slots, each served by a PERSISTENT workgroup on
 * the device that polls its slot in pinned memory.  mrk_serve_rank is then the whole request path, callable from any
 * number of host threads: the request is resolved on the calling thread and written into a free slot; the workgroup
 * assembles, scores and orders it and writes scores / order / status back into pinned memory - no launch, no copy
 * command, no HIP call.  Results and errors are exactly mrk_rank's.  Requests the one-workgroup path does not take
 * (more than 128 candidates, per-item field overrides, a model with a request-normalised column, all slots busy) go
 * through mrk_rank transparently.  A workgroup that has seen no request for a while (2 ms; MRK_SERVE_IDLE_US) leaves
 * its CU and is relaunched by the next request; store flushes stop the workgroups for their duration.
 * n_slots (1 .. 64): the slots are launched in GANGS - one kernel of up to 8 workgroups per stream, workgroup i serving slot i of
 * its gang - because a resident kernel occupies its stream's hardware queue while it stays and a process has few of those
 * (GPU_MAX_HW_QUEUES; the library sets it to 24 before its first HIP call unless the host has set it): 64 slots take 8 streams.
 * A gang leaves as a whole (idle: no request in any of its slots for MRK_SERVE_IDLE_US; old: MRK_SERVE_LIFE_US; told: a store
 * flush) and is launched again as a whole by the next request that finds its slot left.  Up to MRK_SERVE_SPIN_CALLERS (8)
 * callers wait for their answer spinning; the callers beyond them sleep through the time the device is known to need
 * (+ MRK_SERVE_SLEEP_EXTRA_US) and spin for the rest - 64 spinning threads are 64 busy CPUs, which a host with a CPU quota does
 * not have.  Callers beyond the slots are combined by mrk_rank's front.
 * While a queue is started, mrk_rank itself answers through it (same model handle and model name, no matrix asked for, at most
 * 128 candidates) and sends the rest through its batching front: a host calls mrk_serve_start once at warm-up and keeps calling
 * mrk_rank from its request fibers.
 * mrk_serve_stats: the first min(n_out, MRK_SERVE_STATS) of {requests through the queue, requests through mrk_rank, workgroup launches; then, summed over the
 * queue's requests, in ns: host resolve + pack, host publish -> acknowledgement, host copy-out, device input copy + cache drops,
 * device ranking, device result write-back; last: the SHADER CYCLES of the device ranking summed the same way - cycles / ns = the
 * clock the requests ran at (a lone workgroup on an otherwise idle device does not see the boost clock)}.
 * Models: any forest.  Trees of <= 16 leaves are scored by the bit-vector scorer; larger trees (XGBoost maxDepth 6 / 8, LightGBM
 * numLeaves > 16) are walked in the request's workgroup over a matrix it assembles in LDS.  What remains is an LDS limit: that
 * matrix (columns x 128 rows x 8 bytes LightGBM / 4 bytes XGBoost), the forest's largest chunk (<= 24 KB) and the leaf values of
 * up to 32 of its trees must fit the workgroup's 128 KB together - else MRK_ERR_UNSUPPORTED, and mrk_last_error names the sizes. */
typedef struct mrk_server mrk_server;
int mrk_serve_start(mrk_ctx *ctx, mrk_model *model, const char *model_name, int n_slots, mrk_server **out);
int mrk_serve_rank(mrk_server *srv, const mrk_request *req, double *out_scores, int32_t *out_order);
#define MRK_SERVE_STATS 10
int mrk_serve_stats(mrk_server *srv, int64_t *out, int n_out);
void mrk_serve_stop(mrk_server *srv);

/* ------------------------------------------------ multi-GPU (RCCL over xGMI) */

/* The path shards without a data-path collective except one: merging score slices (the reference has
 * no counterpart - one rerank per JVM thread, M/ml/Ranker.scala:27-83).  One process per GPU, one context each; rank
 * 0 draws an id (ncclGetUniqueId) and hands its 128 bytes to the other ranks over any channel the host has, then
 * every rank calls mrk_comm_init (ncclCommInitRank: collective, blocks until all `world` ranks have called it). */
#define MRK_COMM_ID_BYTES 128
int mrk_comm_unique_id(uint8_t *out_id /* MRK_COMM_ID_BYTES */);
int mrk_comm_init(mrk_ctx *ctx, const uint8_t *id, int rank, int world);
/* The same for ranks that live in ONE process: ctxs[i] becomes rank i of a world of n (ncclCommInitRank per context inside
 * ncclGroupStart / ncclGroupEnd - no id to pass around).  One rank per GPU: two contexts on the same ordinal are
 * MRK_ERR_INVALID_ARG.  Afterwards each context's host thread issues the collective calls below like a rank of a
 * multi-process job. */
int mrk_comm_init_local(mrk_ctx *const *ctxs, int n);
int mrk_comm_rank(mrk_ctx *ctx);   /* 0 without a communicator */
int mrk_comm_world(mrk_ctx *ctx);  /* 1 without a communicator */
/* host-value collectives for drivers: max over the ranks (in place), and a barrier */
int mrk_comm_max_f64(mrk_ctx *ctx, double *value);
int mrk_comm_barrier(mrk_ctx *ctx);
/* Item-sharded rank of a batch over the communicator's ranks (every rank holds the same batch and a replica of the
 * store): this rank's slice is assembled and scored (mrk_batch_run_shard with the communicator's rank / world), ONE
 * in-place ncclAllGather of the score slices on the batch's stream, then the sort - every rank ends up with all scores
 * and the order.  Per-request status words are merged too (an item that fails its request - dim mismatch, an XGBoost inf -
 * sits in ONE rank's slice: the words of all ranks are all-gathered and OR-ed before the sort, so every rank reports what
 * the single-GPU path reports).  Asynchronous like mrk_batch_run.  Without a communicator it is mrk_batch_run.
 * COLLECTIVE ORDER: all ranks must issue the collectives of a communicator (these calls, mrk_comm_max_f64, _barrier) in
 * the same order; the library serialises them per context, so driving several batches from several host threads is safe
 * only if every rank runs them in one agreed order. */
int mrk_batch_run_sharded(mrk_batch *batch, mrk_model *model);
/* the all-gather step alone: after mrk_batch_run_shard(batch, model, mrk_comm_rank, mrk_comm_world) on every rank */
int mrk_batch_allgather_scores(mrk_batch *batch);
/* Request-sharded replicas (every rank ranks its own batch of the same size): the scores of all ranks in one device
 * buffer owned by the batch, rank r's at [r * total_items, (r + 1) * total_items); asynchronous on the batch's stream. */
int mrk_batch_gather_scores(mrk_batch *batch, double **d_all_scores);

/* -------------------------------------------------------------- utilities */

int mrk_sync(mrk_ctx *ctx);            /* hipStreamSynchronize on the context stream */
void *mrk_stream(mrk_ctx *ctx);        /* the hipStream_t all work is enqueued on     */

/* HIP-event timing of the kernels launched by the last mrk_batch_run / predict call on this ctx.
 * names: scorer "score", assembly "assemble", request pre-pass "prepass", sort "sort".
 * Enable with mrk_profile_enable(ctx, 1); returns accumulated ms and launch count since enable. */
int mrk_profile_enable(mrk_ctx *ctx, int on);
int mrk_profile_get(mrk_ctx *ctx, const char *kernel, double *total_ms, int64_t *launches);

/* ---- text encoders (BASELINE config 5) ------------------------------------------------------------
 * Replaces ml/onnx/sbert/OnnxSession.scala:29-57 (load), OnnxBiEncoder.scala:13-60 (embed + masked mean pool) and
 * OnnxCrossEncoder.scala:22-51 (pair logits).  The tokenizer is host code and needs no device. */
typedef struct mrk_tokenizer mrk_tokenizer;
typedef struct mrk_encoder mrk_encoder;

/* HuggingFaceTokenizer.newInstance(tokenizer.json, {padding: true, truncation: true}) -- OnnxSession.scala:42-43.
 * BERT WordPiece pipelines only; other pipelines -> MRK_ERR_UNSUPPORTED. */
int mrk_tokenizer_load(const char *tokenizer_json, size_t len, mrk_tokenizer **out);
/* tokenizer.batchEncode(a) / batchEncode(PairList(a, b)): rows padded to the longest row of the batch.  `b` may be
 * NULL.  ids/type_ids/mask are n x capacity row-major with row stride *seq_len on return; MRK_ERR_INVALID_ARG when
 * capacity < longest row (then *seq_len holds the length needed). */
int mrk_tokenizer_encode_batch(mrk_tokenizer *tok, const char *const *a, const char *const *b, int n, int32_t *ids,
                               int32_t *type_ids, int32_t *mask, int capacity, int *seq_len);
void mrk_tokenizer_free(mrk_tokenizer *tok);

typedef struct mrk_encoder_info {
  int32_t layers, hidden, heads, intermediate, vocab, max_positions, type_vocab;
  int32_t has_classifier; /* pooler + 1-logit classifier present (cross-encoder) */
  int32_t max_length;     /* tokenizer truncation length */
  int64_t device_bytes;
  double layer_norm_eps;
} mrk_encoder_info;

/* env.createSession(modelBytes) + the tokenizer -- OnnxSession.scala:42-56.  `weights` is the model file the reference
 * reads (`pytorch_model.onnx`: the initializers of a BERT-family graph are extracted) or the same checkpoint as
 * `model.safetensors`; detected by content.  `heads` = number of attention heads (0: read it from the graph's
 * reshape constants / the safetensors metadata key "num_attention_heads").  Arithmetic: MRK_ENCODER_F32 (below) - the
 * reference's session is an fp32 onnxruntime session, and scores within 1e-5 / the same order need its arithmetic. */
int mrk_encoder_load(mrk_ctx *ctx, const uint8_t *weights, size_t len, const char *tokenizer_json, size_t tok_len,
                     int heads, mrk_encoder **out);
/* The same with the arithmetic chosen by the caller - a property of the handle, never of the size of a call.
 * MRK_ENCODER_F32 (what mrk_encoder_load uses since ABI 8): f32 weights, every matrix product and the attention on the
 * f32-input matrix instruction (v_mfma_f32_16x16x4_f32: exact f32, bit for bit a chain of fma's), libm erf / exp - the
 * arithmetic of the reference's fp32 ONNX session (onnxruntime on the CPU, OnnxSession.scala:42-56); cosines within 1e-5 of
 * transformers' fp32 output (the reference's own tests accept 1e-3, OnnxBiencoderTest.scala:23-25).  Every f32 kernel walks
 * k in one canonical order from a zero accumulator, so a sequence's embedding is the same BITS alone (mrk_rank), in a packed
 * batch of thousands (mrk_batch_*), padded or packed: a request's scores do not depend on the load it arrived under.
 * About 3.5x the time of the fp16 path per packed batch (52 % of the 157 TFLOP/s f32 matrix peak), the same latency for
 * a single query.
 * MRK_ENCODER_FP16 (opt-in; BASELINE config 5's "fp16"): fp16 weights and operands on the matrix cores, f32 accumulation -
 * pooled cosines within 3e-3 of an fp32 run of the graph; about 1 % of a 500-tree forest's scores move by more than 1e-5 and
 * a third of the requests see a pair of candidates swapped (bench.py's config-5 line reports it per run).
 * MRK_ENCODER_AUTO: accepted for hosts built against ABI <= 7 (where it chose by call size); it is MRK_ENCODER_F32 now. */
enum { MRK_ENCODER_FP16 = 0, MRK_ENCODER_F32 = 1, MRK_ENCODER_AUTO = 2 };
int mrk_encoder_load_ex(mrk_ctx *ctx, const uint8_t *weights, size_t len, const char *tokenizer_json, size_t tok_len, int heads,
                        int precision, mrk_encoder **out);
int mrk_encoder_get_info(mrk_encoder *enc, mrk_encoder_info *info);
/* Host-only view of what mrk_encoder_load reads from a model file: writes a JSON object
 * {"heads": h, "tensors": {name: {"shape": [...], "sum": s, "abs_sum": a}}} (BertModel state_dict names, Linear weights
 * as [out, in]) into `out`; MRK_ERR_INVALID_ARG with *needed set when `cap` is too small. No device needed. */
int mrk_checkpoint_describe(const uint8_t *weights, size_t len, char *out, size_t cap, size_t *needed);
/* OnnxBiEncoder.embed: n texts -> n x hidden f32 (masked mean over tokens, f64 accumulation, no normalisation) */
int mrk_encoder_embed(mrk_encoder *enc, const char *const *texts, int n, float *out);
/* same from token ids (n x seq_len, as mrk_tokenizer_encode_batch returns them) */
int mrk_encoder_embed_ids(mrk_encoder *enc, const int32_t *ids, const int32_t *type_ids, const int32_t *mask, int n,
                          int seq_len, float *out);
/* last_hidden_state (output 0 of the graph) for parity checks: n x seq_len x hidden f32 */
int mrk_encoder_hidden_ids(mrk_encoder *enc, const int32_t *ids, const int32_t *type_ids, const int32_t *mask, int n,
                           int seq_len, float *out);
/* OnnxCrossEncoder.encode: n (a, b) pairs -> n logits; MRK_ERR_UNSUPPORTED without a classifier head */
int mrk_encoder_score_pairs(mrk_encoder *enc, const char *const *a, const char *const *b, int n, float *out);
int mrk_encoder_score_ids(mrk_encoder *enc, const int32_t *ids, const int32_t *type_ids, const int32_t *mask, int n,
                          int seq_len, float *out);
void mrk_encoder_free(mrk_encoder *enc);
/* FieldMatchBiencoderSchema.create / FieldMatchCrossEncoderSchema.create with `method.model` set
 * (feature/FieldMatchBiencoderFeature.scala:118-124, FieldMatchCrossEncoderFeature.scala:131-135): from now on
 * mrk_rank / mrk_batch_prepare encode the request's `rankingField` text with this encoder (queries are cached by
 * text, as EmbeddingCache does) instead of expecting a host-computed embedding. */
int mrk_config_bind_encoder(mrk_ctx *ctx, const char *feature, mrk_encoder *enc);

/* ---- field_match term / ngram / bm25 on the device ---------------------------------------------------------------------
 * M/feature/FieldMatchFeature.scala:60-92, M/feature/matcher/FieldMatcher.scala:15-49, BM25Matcher.scala:26-40.
 * Opt-in per feature: the library-level key "match": "device" in the feature's JSON, beside the reference's rankingField /
 * itemField / method {type, language, n, termFreq}.  Without the key a field_match feature is a host-computed column whose
 * per-item values arrive as item field "__ext:<name>", as before.  With it (method.type term | ngram | bm25, anything else
 * is MRK_ERR_PARSE; dim 1):
 *   - state: the item-scope string list "<name>_<itemField.field>" - what FieldMatchFeature.writes puts, matcher.tokenize's
 *     output, strictly ascending in String.compareTo (UTF-16 code unit) order.  A string list that is not, put into such a
 *     column through mrk_store_put_string_list or mrk_store_put_binary, is refused with MRK_ERR_UNSUPPORTED.
 *   - query: matcher.tokenize(request field), computed by the host (the Lucene analyzers stay on the JVM), as the ranking-level
 *     MRK_FIELD_STRING_LIST field "__tokens:<name>".  Absent field (or another type): every item 0.0.  Tokens that are not
 *     strictly ascending fail the request with MRK_ERR_INVALID_ARG; more than MRK_MATCH_MAX_QUERY_TOKENS (term / ngram) or
 *     MRK_MATCH_MAX_QUERY_TOKENS_BM25 (bm25) with MRK_ERR_UNSUPPORTED - a query is never truncated.
 *   - value: term / ngram |Q n D| / |Q u D| (0.0 for an empty query, an unknown item, missing or non-list state, an empty
 *     list); bm25 the sum over the query tokens present in the list, in query order, of
 *     (idf * 2.2) / (1.0 + 1.2 * (0.25 + 0.75 * (len / avgdl))), every operation rounded on its own, idf =
 *     log(1.0 + (docs - gtf + 0.5) / (gtf + 0.5)) with the host's libm log. */
#define MRK_MATCH_MAX_QUERY_TOKENS 128
#define MRK_MATCH_MAX_QUERY_TOKENS_BM25 64
/* BM25MatcherType.create's TermFreqDic.fromFile: `json_bytes` is the dictionary's JSON {"language", "fields", "docs", "avgdl",
 * "termfreq": {term: count}} (BM25Matcher.scala:45), read - and un-gzipped - by the host.  Binds it to the device-matched bm25
 * feature `feature`; may be called again to replace it (requests in flight finish with the old one).  MRK_ERR_PARSE: malformed
 * JSON, a missing key, docs < 0, avgdl not finite or not positive, a count that is not an Int >= 0; MRK_ERR_NOT_FOUND: unknown
 * feature; MRK_ERR_UNSUPPORTED: not a device-matched bm25 field_match.  Ranking a model whose bm25 feature has no
 * dictionary fails with MRK_ERR_INVALID_ARG.  No device needed. */
int mrk_config_bind_termfreq(mrk_ctx *ctx, const char *feature, const char *json_bytes, size_t len);

/* ---- similar items (POST /recommend/<model>): an exact nearest-neighbour index on the device ----------------------------
 * Replaces the HNSW index behind the reference's `similar` (ALS factors) and `semantic` (BERT embeddings) recommenders:
 * M/ml/recommend/embedding/HnswJavaIndex.scala:23-59 (KnnIndexReader.lookup), :68-87 (KnnIndexWriter.write),
 * M/ml/recommend/MFRecommender.scala:66-80 (EmbeddingSimilarityModel.predict), M/ml/Recommender.scala:36-44.  The distance is
 * hnswlib-core's DOUBLE_COSINE_DISTANCE, in f64, every sum walked in dimension order with separate multiplies and adds:
 *   dot += u[i]*v[i]; nru += u[i]*u[i]; nrv += v[i]*v[i];   distance = 1.0 - dot / (sqrt(nru) * sqrt(nrv))
 * The device scans the whole table, so the result is the TRUE n nearest rows (HNSW approximates them), ordered by
 * java.lang.Double.compare on the distance (-0.0 before 0.0, NaN last) and, among equal distances, by ascending row (HNSW
 * defines no tie order; this one is the library's).  Zero vectors are legal (their distance is NaN, returned as the canonical
 * NaN 0x7ff8000000000000); non-finite values follow IEEE arithmetic, nothing is refused.  Results are independent of how many
 * queries share a call.  Limits (MRK_ERR_INVALID_ARG): n + n_items <= 2048, 1 <= cols <= 4096, rows < 2^31.
 * There is no save / load: the host rebuilds the index from its EmbeddingMap (KnnIndex.write / load). */
typedef struct mrk_index mrk_index;
/* KnnIndexWriter.write(EmbeddingMap) -- HnswJavaIndex.scala:68-87: ids[rows] (each stored once), values row-major rows x cols,
 * elem_bytes 4 (float) or 8 (double).  Everything is copied.  The table is stored as f32 when every value survives
 * double -> float -> double unchanged (always true for encoder embeddings, which the reference widens from floats,
 * M/ml/recommend/BertSemanticRecommender.scala:61-66) and as f64 otherwise; both widths give the same bits. */
int mrk_index_build(mrk_ctx *ctx, const char *const *ids, const void *values, int elem_bytes, int64_t rows, int cols, mrk_index **out);
/* EmbeddingMap.rows / .cols, the stored width (4 or 8) and the bytes held on the device; any output may be NULL */
int mrk_index_info(mrk_index *ix, int64_t *rows, int *cols, int *stored_elem_bytes, int64_t *device_bytes);
/* EmbeddingMap.ids(row): NULL when out of range; valid until mrk_index_free */
const char *mrk_index_id(mrk_index *ix, int64_t row);
/* index.get(id) -- HnswJavaIndex.scala:29: the row of an id, -1 when unknown */
int64_t mrk_index_row(mrk_index *ix, const char *id);
/* HnswIndexReader.lookupOne = index.findNearest(vector, n) -- HnswJavaIndex.scala:56-59 -- for n_queries raw vectors
 * (n_queries x cols doubles): out_rows / out_dist are n_queries x n row-major, the first out_n[q] = min(n, rows) entries of
 * row q are filled, nearest first.  Calls of any size are cut into launches inside the library. */
int mrk_index_search(mrk_index *ix, const double *queries, int n_queries, int n, int32_t *out_rows, double *out_dist, int32_t *out_n);
/* KnnIndexReader.lookup(items, n) -- HnswJavaIndex.scala:25-38: no items -> nothing; one item -> the neighbours of its stored
 * vector, nothing when the id is unknown; several -> unknown ids are dropped, duplicates kept, and the query is the centroid
 * (:40-54: per dimension the f64 sum in request order divided by the number kept).  When NO id of a several-item request is
 * known the reference searches for a NaN centroid, whose result is undefined; here that returns nothing.  out_rows / out_dist
 * hold n entries, *out_n are filled. */
int mrk_index_lookup(mrk_index *ix, const char *const *item_ids, int n_items, int n, int32_t *out_rows, double *out_dist, int32_t *out_n);
/* EmbeddingSimilarityModel.predict -- MFRecommender.scala:67-77 -- and the ordering of Recommender.recommend --
 * Recommender.scala:42: lookup(items, count + n_items), drop every result that is one of the request's items, take(count),
 * then the stable sortBy(-score) with score = distance: the response is the `count` nearest items FARTHEST FIRST (NaN scores
 * last).  That is what the reference answers; it is reproduced, not corrected.  out_rows / out_score hold count entries.
 * No items -> MRK_ERR_INVALID_ARG ("similar items recommender requires request.items to be non-empty", :69); nothing left
 * after the filter -> MRK_ERR_NOT_FOUND ("empty response from the recommender", :74). */
int mrk_index_recommend(mrk_index *ix, const char *const *item_ids, int n_items, int count, int32_t *out_rows, double *out_score, int32_t *out_n);
/* BertSemanticPredictor.fit -- M/ml/recommend/BertSemanticRecommender.scala:25-79 -- for a whole catalogue: texts[r] is item r's
 * text fields already joined by the host (" ".join, :54-59); every text is embedded by `enc` (mean pooling, as mrk_encoder_embed)
 * and becomes row r of an ordinary index of cols = hidden, stored as f32, under ids[r] (each stored once).  The catalogue runs
 * through the device in pieces: consecutive texts whose token count (one truncated sequence with its special tokens) sums to at
 * most max_tokens, at most 65 535 texts each, always at least one; 0 = the library's default (131 072), values above 2^24 are
 * taken as 2^24.  Windows of a few pieces run in length order; every row still lands at its input position.  No embedding passes through host memory, and the host tokenises the next piece while the device works on
 * the current one.  The encoder's activation scratch grows to min(max_tokens, total tokens) tokens and stays with the handle.
 * With an encoder of precision f32 (the default) every row has the bits mrk_encoder_embed gives that text alone, whatever
 * max_tokens is; with precision fp16 that holds against one mrk_encoder_embed call of the same texts when the catalogue is one
 * piece, and is not promised across pieces.  Other calls on `enc` from other threads are served between two pieces.
 * MRK_ERR_INVALID_ARG, before any device work: a null ctx / enc / out, an encoder of another context, max_tokens < 0, a null
 * texts[r] or ids[r] (the message names the row), a duplicate id, rows outside mrk_index_build's limit.  On any error *out is
 * NULL and the encoder stays usable.  Everything is copied. */
int mrk_index_build_texts(mrk_ctx *ctx, mrk_encoder *enc, const char *const *ids, const char *const *texts, int64_t rows, int64_t max_tokens,
                          mrk_index **out);
/* index.get(id).vector -- HnswJavaIndex.scala:29-31 -- for n rows: out is n x cols doubles, the stored values widened (exact).
 * A row outside [0, rows) is MRK_ERR_INVALID_ARG and nothing is written. */
int mrk_index_vectors(mrk_index *ix, const int64_t *rows, int n, double *out);
void mrk_index_free(mrk_index *ix);

/* ---- trending items (POST /recommend/<model>, type: trending): the fit on the device ---------------------------------------
 * Replaces TrendingPredictor.fit / load and TrendingModel.predict / save, M/ml/recommend/TrendingRecommender.scala:39-133.
 * Input: the ordered stream of ItemInteraction(item, type, ts) of :42 - ts is the CLICK-THROUGH's ranking timestamp (ct.ct.ts),
 * not the interaction's own; the config's `selector` is applied by the host before it hands interactions over.  Semantics,
 * all bit-exact:
 *   now    = the maximal ts of ALL interactions (:45), types no weight names included
 *   items  = the distinct item ids in order of first appearance (:47); one whose interactions match no weight scores 0.0
 *   per weight w: an interaction counts iff type == w.interaction and ts > now - window.toMillis (:52-53, strict); its bucket is
 *            (now - ts) / 86 400 000 (:57).  A bucket >= window.toDays - a window that is no whole number of days, or shorter
 *            than a day - is the JVM's ArrayIndexOutOfBounds (:58-59): the fit fails with MRK_ERR_DIM_MISMATCH naming the
 *            weight; nothing is clamped or dropped.
 *   part_w = +0.0 for an item without a counted interaction (:79), else (s = 0.0; for every day i in order: s = s +
 *            (double)count[i] * pow(decay, i)) * weight (:72-78) - each * and + one IEEE f64 operation, never fused; pow is the
 *            host libm's.  A day with no count is still visited: 0 * Infinity is NaN, as on the JVM.
 *   score  = the parts summed left to right in config order starting from the first (Scala 2.13's List.sum as a reduce; 0.0
 *            for no weights) (:82)
 *   model  = the items by stable sortBy(-score) (:85): java.lang.Double.compare on the negated score - +0.0 before -0.0, NaN
 *            last -, ties in order of first appearance.  Recommender.recommend's second sortBy(-score) (M/ml/Recommender.scala:42)
 *            is the identity on this list, so predict's answer is the response.
 * Refused rather than imitated: two weights naming one interaction (the reference's .toMap lets the last one's counts feed
 * both), more than 2^31 - 1 interactions, a count table (4 B x items x sum of window days) that does not fit the device memory
 * free at fit - all MRK_ERR_UNSUPPORTED.  A finished model is a host object: predict, id, save and load read no device memory. */
typedef struct mrk_trending_builder mrk_trending_builder;
typedef struct mrk_trending mrk_trending;
/* TrendingConfig's decoder, :137-164: {"weights":[{"interaction":"click","weight":1.0,"decay":0.5,"window":"30d"}, ...]} with the
 * reference's defaults (1.0, 1.0, 30d); durations are ([0-9]+)([smhd]).  MRK_ERR_PARSE for malformed JSON or a bad duration,
 * MRK_ERR_UNSUPPORTED for a duplicate interaction - both judged before the context is looked at. */
int mrk_trending_begin(mrk_ctx *ctx, const char *config_json, mrk_trending_builder **out);
/* The flatMap of :40-44: appends n interactions in order.  item_ids[n]; type_idx[n] indexes THIS call's type_names[n_types];
 * ts_ms[n].  May be called any number of times; the result does not depend on how the stream is cut into calls.  An index
 * outside the table or a null id fails the call with MRK_ERR_INVALID_ARG and nothing of it is appended. */
int mrk_trending_add(mrk_trending_builder *b, const char *const *item_ids, const char *const *type_names, int n_types, const int32_t *type_idx,
                     const int64_t *ts_ms, int64_t n);
/* The rest of TrendingPredictor.fit, :45-86.  No interactions: MRK_ERR_NOT_FOUND ("no interactions found").  The builder stays
 * valid and can take more adds; a later fit covers everything added so far. */
int mrk_trending_fit(mrk_trending_builder *b, mrk_trending **out);
void mrk_trending_builder_free(mrk_trending_builder *b);
/* TrendingPredictor.loadSync, :90-110: big-endian i32 1, i32 size, per item readUTF + f64.  Ids are kept as the bytes readUTF's
 * length covers (modified UTF-8, as mrk_store_put_binary keeps them).  Another version: MRK_ERR_UNSUPPORTED; size <= 0,
 * truncation or trailing bytes: MRK_ERR_PARSE.  No device needed; ctx may be NULL. */
int mrk_trending_load(mrk_ctx *ctx, const uint8_t *bytes, size_t len, mrk_trending **out);
/* TrendingModel.save, :123-133.  MRK_ERR_INVALID_ARG with *needed set when `out` is NULL or `cap` too small; an id of more than
 * 65 535 bytes is what writeUTF throws on: MRK_ERR_UNSUPPORTED. */
int mrk_trending_save(mrk_trending *t, uint8_t *out, size_t cap, size_t *needed);
/* items of the model, interactions and `now` of its fit (-1 / -1 for a loaded model); any output may be NULL */
int mrk_trending_info(mrk_trending *t, int64_t *items, int64_t *interactions, int64_t *now_ms);
/* the id at place `rank` of the model: NULL when out of range; valid until mrk_trending_free */
const char *mrk_trending_id(mrk_trending *t, int64_t rank);
/* TrendingModel.predict, :116-121: the scores of the first *out_n = min(count, items) items; their ids are ranks 0 .. *out_n - 1.
 * count <= 0: MRK_ERR_INVALID_ARG ("count should be greater than 0"). */
int mrk_trending_predict(mrk_trending *t, int count, double *out_scores, int32_t *out_n);
void mrk_trending_free(mrk_trending *t);

/* ---- similar items (POST /recommend/<model>, type: als): the fit on the device ---------------------------------------------
 * Replaces MFPredictor.fit (M/ml/recommend/MFRecommender.scala:26-37) with ALSRecImpl.train (M/ml/recommend/mf/ALSRecImpl.scala:
 * 18-41): the item factors of an element-wise ALS over the click-through history, written straight into an ordinary mrk_index.
 * The reference runs librec's EALSRecommender, which is not part of it; what is computed here is the algorithm that class
 * implements - He, Zhang, Kan, Chua, "Fast Matrix Factorization for Online Recommendation with Implicit Feedback", SIGIR 2016,
 * Algorithm 1, Eq. 12-13 - with the reference's fixed settings (:20-32): eALS (rec.eals.wrmf.judge = 1), w0 = 128, alpha = 0.4,
 * every rating and every positive weight 1.  This is a stated definition, not a parity claim against librec (DESIGN.md
 * section 17, "Unpinned").  Semantics, all f64, every * + / one IEEE operation:
 *   input  = one (user, item) per line of MFPredictor.uirt (MFRecommender.scala:54-59); the host applies the selector, the
 *            `interactions` type filter (:61-63) and the no-user rule before it hands pairs over.  Users and items are numbered in
 *            order of first appearance over all adds; duplicate pairs count once.  R_u = the items of user u ascending, R_i = the
 *            users of item i ascending, nnz = the distinct pairs, n_i = |R_i|.
 *   c_i    = (w0 * p_i^alpha) / Z, p_i = n_i / nnz, Z = the p_j^alpha summed in item order; pow is the host libm's.
 *   init   = the caller's matrices, or value(seed, matrix, row, col) of the library's counter-based generator (Gaussian, mean 0,
 *            standard deviation 0.01; mrk_als_init_matrix returns the same bytes).
 *   one iteration = S^q[f][k] = sum_i c_i * (q_if * q_ik);  for every user u: r_j = p_u . q_i (k in order) for its entries, then
 *            for f = 0 .. K-1 in order:  rf_j = r_j - p_uf * q_if;  num = sum_j (1.0 - (1.0 - c_i) * rf_j) * q_if;
 *            den = sum_j (1.0 - c_i) * (q_if * q_if);  ks = sum_k (k == f ? 0.0 : p_uk * S^q[f][k]);
 *            p_uf = (num - ks) / ((den + S^q[f][f]) + lambda_u);  r_j = rf_j + p_uf * q_if.
 *            Then S^p[f][k] = sum_u p_uf * p_uk and for every item i the same with the roles exchanged and the S terms weighed by
 *            the row's c_i:  q_if = (num - c_i * ks) / ((den + c_i * S^p[f][f]) + lambda_i).
 *   order of every sum: a function of its length alone, written out in DESIGN.md section 17 and restated by
 *            tests/als_reference.py; the result has that restatement's bits and two fits of one input are identical.
 *   result = an mrk_index of rows = items (in order of first appearance), cols = factors, stored as f64 (EmbeddingMap,
 *            M/ml/recommend/embedding/EmbeddingMap.scala:10-19); the factors never visit host memory.
 * Limits, all MRK_ERR_UNSUPPORTED with the sizes in mrk_last_error: factors > 256; more than 2^31 - 1 pairs; more items than an
 * index has rows; working memory that does not fit what is free on the device at fit.  One device per fit. */
typedef struct mrk_als_builder mrk_als_builder;
/* ALSConfig's decoder, ALSRecImpl.scala:60-81, with the reference's defaults (:46-54): iterations 100, factors 100, userReg and
 * itemReg 0.01f.  The item regulariser is read from the key "itemRef" (:66) - a key "itemReg" is IGNORED, as in the reference;
 * reproduced, not corrected.  Both regularisers are Java floats: their value in the arithmetic is (double)(float)x.
 * `interactions`, `store` and `selector` are the host's.  MRK_ERR_PARSE for malformed JSON or a field of the wrong type,
 * MRK_ERR_INVALID_ARG for factors or iterations < 1 - both judged before the context is looked at. */
int mrk_als_begin(mrk_ctx *ctx, const char *config_json, mrk_als_builder **out);
/* The same builder without a context: add, info, config, id and problem work (no device is touched); fit is MRK_ERR_INVALID_ARG. */
int mrk_als_begin_host(const char *config_json, mrk_als_builder **out);
/* Appends n pairs, user_ids[n] / item_ids[n], in order (the lines of :54-59).  May be called any number of times; the result does
 * not depend on how the stream is cut into calls.  A null id fails the call with MRK_ERR_INVALID_ARG and nothing of it is
 * appended. */
int mrk_als_add(mrk_als_builder *b, const char *const *user_ids, const char *const *item_ids, int64_t n);
/* ALSRecImpl.train + KnnIndex.write (MFRecommender.scala:31-32).  init_users (users x factors) and init_items (items x factors),
 * row-major f64: both or neither (one of the two: MRK_ERR_INVALID_ARG); neither: the generator with `seed`.  out_user_factors
 * (nullable, users x factors) receives the final user factors, which the reference discards.  No pairs: MRK_ERR_NOT_FOUND.  On
 * any error *out is NULL.  The builder stays valid for more adds and later fits; *out is freed with mrk_index_free. */
int mrk_als_fit(mrk_als_builder *b, uint64_t seed, const double *init_users, const double *init_items, double *out_user_factors, mrk_index **out);
/* distinct users and items, pairs added and distinct pairs so far; any output may be NULL */
int mrk_als_info(mrk_als_builder *b, int64_t *users, int64_t *items, int64_t *pairs, int64_t *distinct_pairs);
/* the decoded config: the regularisers as the doubles the arithmetic uses; any output may be NULL */
int mrk_als_config(mrk_als_builder *b, int *iterations, int *factors, double *lambda_user, double *lambda_item);
/* the id with inner index `index` of matrix 0 (users) / 1 (items): NULL when out of range; valid until the builder is freed */
const char *mrk_als_id(mrk_als_builder *b, int matrix, int64_t index);
/* What a fit would iterate over (host only): R_u as CSR (user_offsets[users + 1], user_items[distinct pairs]), R_i as CSC
 * (item_offsets[items + 1], item_users[distinct pairs]) and c_i (confidence[items]); any output may be NULL.  No pairs:
 * MRK_ERR_NOT_FOUND. */
int mrk_als_problem(mrk_als_builder *b, int32_t *user_offsets, int32_t *user_items, int32_t *item_offsets, int32_t *item_users, double *confidence);
/* The generator of the initial factors (host only): out = rows x cols values of matrix 0 (users) / 1 (items), each a function of
 * (seed, matrix, row, column) alone (csrc/als_host.hpp states it). */
int mrk_als_init_matrix(uint64_t seed, int matrix, int64_t rows, int cols, double *out);
void mrk_als_builder_free(mrk_als_builder *b);

/* ---- Evaluation on held-out click-throughs: the step that ends every `metarank train` --------------------------------------------
 * LambdaMARTModel.eval (M/ml/rank/LambdaMARTRanker.scala:406-445, called at :115-123): every group of the test split scored,
 * ordered by score and reduced to NDCG@k / MAP@k / MRR, beside two baselines - the unchanged request order ("noop") and random
 * scores.  Groups are sorted and summed on the device (csrc/eval.hip), thousands per launch; new symbols only, no new struct.
 * PINNED by the reference tree and followed exactly: NDCG(cutoff, nolabels = 1.0, relpow = true) with the default ndcg@10, one
 * predictMat per group (scoring is per row: one pass over all rows gives the same scores), noopArray(len)(i) = (len - i) /
 * len.toDouble, the mean over groups.
 * ASSUMPTION (ltrlib's metric.{NDCG,MAP,MRR} sources are not in the reference tree): the formulas are this
 * project's.  Per group of n items with scores s and labels y, k = cutoff == 0 ? n : min(cutoff, n):
 *   order  pi = the stable descending order of sortBy(-score), as /rank answers: NaN scores last, +0.0 before -0.0, ties in
 *          group order.
 *   NDCG   ASSUMPTION: gain(y) = y, or 2^y - 1 with MRK_EVAL_RELPOW; dcg = sum over i < k of gain(y[pi(i)]) / log2(i + 2), added
 *          one after the other for i = 0, 1, ... in f64 (every / and + correctly rounded, never fused; the first term starts the
 *          sum); idcg = the same sum over the gains sorted descending; the value is `nolabels` when idcg == 0, else dcg / idcg.
 *          log2 and 2^y are the HOST's libm (std::log2, std::pow): for a label whose 2^y is not exactly representable the value
 *          follows that libm.
 *   MAP    ASSUMPTION: an item is relevant when y > 0; ap = (sum over relevant positions i < k of hits_i / (i + 1)) / min(R, k),
 *          hits_i = relevant items among pi(0..i), R = relevant items of the group; integers converted to f64, the sum in
 *          position order; 0.0 when R == 0.
 *   MRR    ASSUMPTION: 1.0 / r, r = the 1-based position in pi of the first relevant item; 0.0 without one.  Ignores the cutoff.
 *   mean   the per-group values added in group order in f64, divided by n_groups.
 * Unverifiable here; tests/eval_reference.py restates them and the device agrees with it bit for bit. */
enum { MRK_METRIC_NDCG = 0, MRK_METRIC_MAP = 1, MRK_METRIC_MRR = 2 };
enum { MRK_EVAL_RELPOW = 1 }; /* flags: NDCG gain = 2^label - 1 instead of label */

/* One metric of caller-supplied scores.  scores / labels: host f64[group_offsets[n_groups]]; group g is
 * [group_offsets[g], group_offsets[g + 1]).  out_value: the mean over groups; out_per_group (nullable): n_groups f64.
 * cutoff == 0: none (the reference's Int.MaxValue).  MRK_ERR_INVALID_ARG, all judged before any device work: a null pointer
 * where one is required, n_groups < 1, a negative cutoff, an unknown metric or flag, offsets that do not start at 0 or do not
 * strictly increase (empty groups are refused, as loadDataset filters them out), a non-finite label.  MRK_ERR_UNSUPPORTED: a
 * group of more than 2^30 items, or arrays that do not fit the device's free memory. */
int mrk_eval_scores(mrk_ctx *ctx, int metric, int cutoff, int flags, double nolabels, const double *scores, const double *labels,
                    const int64_t *group_offsets, int64_t n_groups, double *out_value, double *out_per_group);

/* LambdaMARTModel.eval: scores rowmajor (group_offsets[n_groups] rows x cols, host) ONCE with the model - uploaded in pieces of
 * about 64 MiB, the matrix never has to fit the device -, then every listed metric for the predicted scores, for noopArray and -
 * if random_scores != NULL (one f64 per row) - for those.  out: n_metrics x 3 f64 (value, noop, random; random = NaN when not
 * given).  out_scores (nullable): one f64 per row, what mrk_model_predict_f64 gives for the matrix.  Errors as above; a matrix
 * with fewer columns than the model splits on is MRK_ERR_DIM_MISMATCH and an infinite cell of an XGBoost matrix
 * MRK_ERR_INVALID_ARG, as predictMat gives. */
int mrk_model_eval(mrk_model *model, const int *metrics, const int *cutoffs, int n_metrics, int flags, double nolabels,
                   const double *rowmajor, int cols, const double *labels, const int64_t *group_offsets, int64_t n_groups,
                   const double *random_scores, double *out, double *out_scores);

/* ---- Training: LambdaMART forests fitted on the device ------------------------------------------------------------------------------
 * LambdaMARTPredictor.makeBooster (M/ml/rank/LambdaMARTRanker.scala:161-190) for the LightGBM backend: the forest comes back as
 * LightGBM's text format (objective=lambdarank) and loads through mrk_model_load like any other.  New symbols only, no new struct.
 * A trainer takes its matrix in one of two ways.  mrk_train_set takes it from HOST memory: a matrix mrk_values wrote is fetched
 * first (mrk_batch_fetch), its bins are found on the host (steps 2, 2x, 2c) and it is uploaded in pieces - it never has to fit the
 * device.  mrk_train_append_device + mrk_train_seal take it from DEVICE memory, where mrk_values wrote it (mrk_batch_device_outputs'
 * d_matrix): the rows stay where they are, and steps 2, 2x and 2c run on the device (step 2d) - the whole matrix must then fit the
 * device beside the fit's working memory, and mrk_train_set stays the fallback when it does not.
 * ASSUMPTIONS (unpinned): neither LightGBM nor its sources are in the reference tree, so this is NOT LightGBM's bit stream.  The
 * algorithm below is this project's: LightGBM's lambdarank objective and leaf-wise histogram learner where the rules are public,
 * and two departures that make every result independent of the order anything arrives in - (a) whatever is summed across rows is
 * an int64 sum of quantised values (no float atomics anywhere), (b) exp and log2 are the HOST's libm, through tables.
 * tests/train_reference.py restates it and the device agrees with that to the bit and the byte.  Config keys and [defaults]:
 * LightGBMConfig's iterations [100], learningRate [0.1], ndcgCutoff [10], maxDepth [8], seed [0], numLeaves [16], sampling [0.8],
 * debias [false; true is MRK_ERR_UNSUPPORTED], and max_bin [255], truncation [30], sigma [1.0], min_data_in_leaf [20],
 * min_sum_hessian [1e-3], lambda_l2 [0], early_stopping [20]; for categorical columns (steps 2c, 5c) categorical [[]: an array of
 * distinct column indices >= 0; one >= cols is MRK_ERR_INVALID_ARG at mrk_train_set], max_cat_to_onehot [4], max_cat_threshold
 * [32], cat_smooth [10.0, > 0], cat_l2 [10.0, >= 0], min_data_per_group [100].  An unknown key is MRK_ERR_PARSE.  Without
 * `categorical` a fit gives the bytes it gave before these keys existed.
 *  1 input     f64 row-major rows x cols; labels integers 0 ... 30; groups under mrk_model_eval's rules, at most 4096 rows each; an
 *              infinite cell is MRK_ERR_INVALID_ARG; the initial score is 0.
 *  2 bins      per column, on the host: v = the sorted non-NaN cells (-0.0 is +0.0), m of them.  At most max_bin - 1 distinct
 *              values: a bound between every two neighbours.  Else for i = 1 ... max_bin - 2 a bound at the first p >=
 *              floor(i * m / (max_bin - 1)) with v[p] != v[p - 1], duplicates dropped.  The bound between a < b is (a + b) / 2 in
 *              f64, or a when that is not below b.  bin(x) = the number of bounds < x (so x <= bound goes left, as the scorers
 *              decide); NaN is bin 255.  A column with one bin never splits.  The validation set uses the same bounds.
 *  2c bins of a categorical column (string features with encode: index and the one-dimensional referer, FeatureMapping.scala:91,
 *              RefererFeature.scala:109: mrk_values_columns' `category`), on the host: the category of a cell is c = (int64) trunc(x);
 *              NaN and c < 0 have none; an infinite cell is MRK_ERR_INVALID_ARG; c > 32764 (the largest id the scorers' categorical
 *              cell holds exactly) is MRK_ERR_UNSUPPORTED, naming column, row and value.  Counted over the TRAINING set, the
 *              min(distinct, max_bin - 1) most frequent categories are kept, ties to the lower id; the bin of a kept category is
 *              its position among the kept ones in ascending id, K of them (the column's nbins).  Everything else is bin 255: NaN,
 *              a negative value, a category not kept (rare, or seen only in the validation set).  Bin 255 of a categorical column
 *              ALWAYS goes right - what CategoricalDecision does with NaN, a negative value and an id outside the bitset - so the
 *              trainer's routing and the model's prediction agree for every possible cell.  Rows are binned on the device through
 *              a dense id -> bin byte table per column (at most 32765 bytes).  The validation set uses the training set's table.
 *  2d bins of a matrix that was appended from device memory (mrk_train_append_device, mrk_train_seal): the device finds the SAME
 *              bounds, bit for bit, and the same kept categories.  The appended pieces are kept column-major; per numeric column
 *              the cells become sort keys (narrowed to f32 for step 2x, -0.0 as +0.0, NaN last), are ordered as (key, row) pairs
 *              - one workgroup up to 4096 cells, the sample sort of the large requests above -, and the positions of steps 2 / 2x
 *              are taken from the sorted cells: over a sorted array the first p >= t with v[p] != v[p - 1] is t itself or the
 *              first index holding a value above v[t], one binary search per bound.  Per categorical column the device counts
 *              ids 0 ... 32764 with integer atomics and the host keeps the most frequent as in step 2c.  The refusals of steps 1,
 *              2x and 2c keep their statuses and name the lowest (column, row) that holds such a cell.  The bins written are the
 *              bytes mrk_train_set writes for the same rows, so the fit and the model are the same too.
 *  3 gradients per group of n rows: pi = the order of mrk_eval_scores; gain(y) = 2^y - 1; k = min(truncation, n); inv = 1 /
 *              (sum over i < k of sorted-descending gain_i / lg[i], added in order from 0.0), 0 when that sum is 0; lg[i] =
 *              log2(i + 2).  A pair of ranks (r, q) counts when the labels differ and min(r, q) < k; with hi / lo the item of the
 *              higher / lower label: delta = s_hi - s_lo; rho = T[clamp((delta - lo) * f, 0, BINS - 1) truncated];
 *              w = ((gain_hi - gain_lo) * |1 / lg[r_hi] - 1 / lg[r_lo]|) * inv; lambda = (sigma * rho) * w;
 *              eta = (((sigma * sigma) * rho) * (1 - rho)) * w; g[hi] -= lambda, g[lo] += lambda, h[both] += eta.  An item adds
 *              its pairs in ascending partner rank from 0.0.  T[t] = 1 / (1 + exp(sigma * (lo + t / f))), BINS =
 *              MRK_TRAIN_SIGMOID_BINS, lo = -25 / sigma, f = BINS / (50 / sigma).  Every operation f64, correctly rounded, never
 *              fused.  No lambdarank_norm, no position debias.
 *  4 quantise  e_g = 61 - bitlen(rows) - E(max |g|), frexp(x) = m * 2^E; q_g = (int64) nearbyint(ldexp(g, e_g)), ties to even; h
 *              likewise with max h.  max |g| == 0 ends training.
 *  5 tree      leaf-wise.  Per leaf and column of the tree's subset a histogram (sum q_g, sum q_h, count) per bin.  Candidates b =
 *              0 ... nbins - 2, left = bins <= b; NaN goes right, and with rows in bin 255 also left.  Real sums are ldexp((double)
 *              Q, -e).  Admitted when both counts >= min_data_in_leaf, both hessian sums >= min_sum_hessian, the leaf's depth <
 *              maxDepth and gain = (GL * GL / (HL + l2) + GR * GR / (HR + l2)) - G * G / (H + l2) > 0.  Best: the highest gain,
 *              then the lowest column, the lowest b, NaN right.  The leaf with the best gain splits (ties: the lowest leaf) until
 *              numLeaves leaves or no candidate.  LightGBM's numbering: split s makes node s, the left child keeps the leaf index,
 *              the right is leaf s + 1.  threshold = the bound of b; decision_type = 8 | (NaN left ? 2 : 0); leaf_value =
 *              (-G / (H + l2)) * learningRate.  A tree that cannot split ends training and is not emitted.
 *  5c categorical column: from the same (sum q_g, sum q_h, count) histogram, every operation f64, correctly rounded, never fused.  A
 *              candidate is a set L of bins < K that goes left; everything else goes right, bin 255 included.
 *              K <= max_cat_to_onehot, one-vs-rest: L = {b} for b < K; gain is step 5's with lambda_l2; admitted as in step 5;
 *              best: the highest gain, then the lowest b.
 *              Else, sorted: a bin is eligible when count >= cat_smooth; its key is G_b / (H_b + cat_smooth); the m eligible bins
 *              ascending by (key, bin) (keys are finite and never -0.0: a total order); max_num = min(max_cat_threshold, (m + 1) /
 *              2); candidates are the first i bins of that order (direction 0) and the last i (direction 1), i = 1 ... max_num;
 *              gain = (GL * GL / (HL + l2c) + GR * GR / (HR + l2c)) - G * G / (H + lambda_l2), l2c = lambda_l2 + cat_l2 (the sides
 *              are regularised by cat_l2, the parent's term is not: LightGBM's rule); admitted when both counts >=
 *              max(min_data_in_leaf, min_data_per_group), both hessian sums >= min_sum_hessian and gain > 0; best: the highest
 *              gain, then direction 0, then the smaller i.
 *              Departures from LightGBM: every prefix is judged on its own (LightGBM's running cnt_cur_group makes a candidate
 *              depend on which earlier ones were skipped; judged alone, 256 lanes take all prefixes at once); leaf values keep
 *              step 5's -G / (H + lambda_l2) * learningRate: cat_l2 does not enter outputs.
 *              Across columns and leaves nothing changes: the highest gain, then the lowest column, a numeric and a categorical
 *              column each with its own gain.  In the text a categorical node has decision_type = 9 (categorical, missing type
 *              NaN), threshold = its ordinal among the tree's categorical nodes; the tree carries num_cat, cat_boundaries and
 *              cat_threshold (u32 words over category IDS, max member id / 32 + 1 words per node); feature_infos of the column is
 *              the kept ids joined by ':' or `none`.  A tree without such a node is written as before.
 *  6 scores    score[row] += leaf_value, in tree order; validation rows walk the tree by their bins.
 *  7 subset    per tree min(cols, max(1, floor(cols * sampling + 0.5))) columns: a partial Fisher-Yates shuffle of 0 ... cols - 1
 *              (position j swaps with j + z % (cols - j), z the next splitmix64 output; state = (uint32) seed << 32 | tree index),
 *              the first ones taken, ascending.  Made on the host.
 *  8 stopping  with a validation set: ndcg@ndcgCutoff (relpow, nolabels = 1.0: mrk_eval_scores' number) after every iteration; the
 *              best iteration is replaced only by a strictly greater value; stops after early_stopping iterations without one;
 *              the model holds the trees up to the best iteration.  Without one: `iterations` trees.
 *
 * backend: "xgboost" - the XGBoostConfig arm of makeBooster (the default backend of a Metarank model, LambdaMARTRanker.scala:461), through
 * the same symbols.  The key "backend" is "lightgbm" [the default: every rule above, byte for byte] or "xgboost"; another string is
 * MRK_ERR_INVALID_ARG, another type MRK_ERR_PARSE.  ASSUMPTIONS (unpinned, as above): neither libxgboost nor its sources are on hand, so its
 * bits are not claimed; treeMethod "exact" enumerates every distinct value, this is a histogram learner over at most 255 bins.  Both
 * reproducibility rules hold unchanged (int64 sums of quantised values; exp and log2 from the host's tables).
 * tests/train_xgb_reference.py restates it and the device agrees to the bit and the byte.  Keys and [defaults]: XGBoostConfig's iterations
 * [100], learningRate [0.1], ndcgCutoff [10], maxDepth [8; 1 ... 15], seed [0], sampling [0.8: the ROW subsample, 0 < s <= 1], debias
 * [false; true is MRK_ERR_UNSUPPORTED], and max_bin [255], truncation [30], sigma [1.0], early_stopping [20], lambda [1.0, >= 0], gamma
 * [0.0, >= 0], min_child_weight [1.0, >= 0].  numLeaves, min_data_in_leaf, min_sum_hessian, lambda_l2, max_cat_to_onehot,
 * max_cat_threshold, cat_smooth, cat_l2 and min_data_per_group are MRK_ERR_INVALID_ARG naming the key (a setting that would do
 * nothing); so are lambda, gamma and min_child_weight under the default backend.  A non-empty `categorical` is MRK_ERR_UNSUPPORTED
 * (set-membership splits in XGBoost JSON are not built; an undeclared category column splits as a number).  Steps 1, 3, 4 and 8 are the
 * ones above; step 3 and step 8's metric read the widened f32 scores of 6x.
 *  2x bins     per column, on the host: the cells are narrowed to f32 (round to nearest even; -0.0f counts as +0.0f); a finite f64 that
 *              narrows to +-inf is MRK_ERR_INVALID_ARG naming column and row (predictMat refuses such a cell), in either set.  v = the
 *              sorted non-NaN narrowed cells; the positions are step 2's.  The bound between neighbours a < b is b ITSELF, an f32:
 *              XGBoost's cut convention is x < cut.  bin(x) = the number of bounds <= (float) x; NaN is bin 255.  Candidate c sends left
 *              exactly the cells with (float) x < bound[c] - the emitted model's own test - so every possible cell, seen in training or
 *              not, is routed the same way by the trainer and by the model.  mrk_train_bins returns these bounds widened to f64.
 *  7x rows     row r is in tree t's sample when sampling >= 1 or (z >> 11) * 2^-53 < sampling, z = the first splitmix64 output from
 *              the state ((uint64) (uint32) seed << 32 | t) ^ (r * 0xD6E8FEB86659FD93).  Computed where it is used; no list exists.  A
 *              row outside the sample adds nothing to any histogram (neither its count nor q_g, q_h); it is still routed and scored.
 *              Every tree sees all columns.
 *  5x tree     level-wise.  The root is node 0.  The open nodes of depth d are taken in ascending id; a node that splits gives its left
 *              child the next free id and its right child the one after: XGBoost's breadth-first numbering.  Per open node and column a
 *              histogram (sum q_g, sum q_h, count) per bin over the SAMPLED rows.  Candidates and the NaN rule are step 5's.  Admitted
 *              when both sides have >= 1 sampled row, HL >= min_child_weight and HR >= min_child_weight, d < maxDepth and gain =
 *              (GL * GL / (HL + lambda) + GR * GR / (HR + lambda)) - G * G / (H + lambda) > gamma; every operation f64, correctly
 *              rounded, never fused, from ldexp((double) Q, -e).  Best per node: the highest gain, then the lowest column, the lowest
 *              bin, NaN right.  EVERY open node with an admitted candidate splits - nodes do not compete -, the others are leaves.
 *              weight = -G / (H + lambda) (H + lambda == 0: MRK_ERR_INVALID_ARG at mrk_train_fit); a leaf's value is (float) (weight *
 *              learningRate).  A tree whose root cannot split ends training and is not emitted.
 *  6x scores   f32, as the model predicts them: s = 0.5f (the base_score), then s = s + leaf in f32, in tree order.  Training rows -
 *              the unsampled ones too - and validation rows take the leaf their bins route them to.  mrk_train_scores returns the
 *              widened value, equal to mrk_model_predict_f64 of the emitted model bit for bit; without a tree every score is 0.5.
 *  model text  XGBoost's JSON as libxgboost 2.1 writes it (version [2,1,0], objective rank:ndcg, base_score "5E-1", num_feature = cols,
 *              empty categorical arrays), no whitespace.  Per tree split_conditions = the bound or the leaf value, base_weights =
 *              (float) weight, loss_changes = (float) gain (0 for a leaf: Booster.weights() works), sum_hessian = (float) H, parents
 *              2147483647 for the root, default_left = NaN goes left, split_type all 0.  Every f32 is printed as %.9g of its widened
 *              value.  mrk_model_load(MRK_BACKEND_XGBOOST) reads it. */
#define MRK_TRAIN_SIGMOID_BINS 65536
typedef struct mrk_trainer mrk_trainer;

/* Parses the config (errors: above) and creates a trainer on ctx's device.  One GPU per fit. */
int mrk_train_begin(mrk_ctx *ctx, const char *config_json, mrk_trainer **out);
/* Hands over a data set: which = 0 the training set, 1 the validation set (optional; after the training set, same cols).  The
 * matrix is binned on the device, uploaded in pieces of about 64 MiB (MRK_TRAIN_PIECE_ROWS=n: pieces of n rows): it need not fit
 * the device, and nothing of the caller's is kept.  MRK_ERR_INVALID_ARG: null pointers, a bad `which`, rows / cols < 1, offsets
 * that do not start at 0 or do not strictly increase, a label that is no integer in 0 ... 30, an infinite cell.
 * MRK_ERR_UNSUPPORTED, with the sizes in mrk_last_error: cols > 65535, rows >= 2^31, a group of more than 4096 rows, working
 * memory (bins, gradients, numLeaves x subset x 256 histogram cells; backend "xgboost": 2 levels x min(2^(maxDepth - 1), rows) nodes x
 * cols x 256 cells of 20 B) beyond what the device has free. */
int mrk_train_set(mrk_trainer *t, int which, const double *rowmajor, int64_t rows, int cols, const double *labels, const int64_t *group_offsets,
                  int64_t n_groups);
/* Step 2d, the matrix from device memory.  Copies rows x cols f64 cells from d_rowmajor - a DEVICE pointer on the trainer's device:
 * a batch's d_matrix (mrk_batch_device_outputs), or d_matrix + first_row * cols to take a range of its rows - into staging the
 * trainer owns (column-major; rows x cols x 8 bytes).  The work that wrote the cells must have finished (mrk_batch_sync); d_rowmajor
 * may be rewritten as soon as the call returns.  Any number of calls per set; the first one fixes cols.  MRK_ERR_INVALID_ARG: a bad
 * `which`, a fitted trainer, a null pointer, rows / cols < 1, cols other than the pieces before.  MRK_ERR_UNSUPPORTED, with the sizes
 * in mrk_last_error: staged rows reaching 2^31, cols > 65535, staging beyond what the device has free (mrk_train_set, which never
 * needs the matrix resident, is the way then).  mrk_train_set(which) drops what was appended to that set and not sealed. */
int mrk_train_append_device(mrk_trainer *t, int which, const double *d_rowmajor, int64_t rows, int cols);
/* Ends an appended set: labels and group_offsets are HOST arrays under mrk_train_set's rules (the offsets end at the number of
 * appended rows), every check and status is mrk_train_set's.  which = 0: finds the bins on the device (step 2d; beside the staging
 * it needs the keys and the sort's scratch of ONE column, about 34 bytes per row), bins the cells and frees the staging.  which = 1:
 * after a training set (from either path, same cols); checks the cells on the device and bins them with the training set's tables.
 * Afterwards the trainer is where mrk_train_set would have left it; a trainer may take one set from the host and the other from the
 * device.  A seal that fails drops the appended rows all the same. */
int mrk_train_seal(mrk_trainer *t, int which, const double *labels, const int64_t *group_offsets, int64_t n_groups);
/* The trainer's bounds of numeric column col of the training set, whichever path found them (backend "xgboost": the f32 bounds
 * widened, as mrk_train_bins returns them): *n_bounds of them, copied when cap >= *n_bounds.  MRK_ERR_INVALID_ARG: a categorical
 * column, a column outside the matrix, no training set yet. */
int mrk_train_bounds(mrk_trainer *t, int col, double *out_bounds, int cap, int *n_bounds);
/* Runs the fit (steps 3 - 8). */
int mrk_train_fit(mrk_trainer *t);
/* The model text (LightGBM's text format, or XGBoost's JSON with backend "xgboost").  *needed: its length in bytes; copies it when cap >= *needed (out may be NULL to ask for the length). */
int mrk_train_model(mrk_trainer *t, void *out, size_t cap, size_t *needed);
/* iterations_run: trees grown; best_iteration: trees in the model; out_metric (nullable): the validation metric after each iteration,
 * min(cap, iterations_run) values (none without a validation set). */
int mrk_train_history(mrk_trainer *t, int *iterations_run, int *best_iteration, double *out_metric, int cap);
/* The trainer's own f64 scores of set `which` at the best iteration: what the model predicts for those rows, bit for bit. */
int mrk_train_scores(mrk_trainer *t, int which, double *out);
void mrk_train_free(mrk_trainer *t);
/* Step 3 alone: out_g / out_h, one f64 per row.  Uses sigma and truncation of the config.  Also a device-side custom objective for a
 * host that keeps lib_lightgbm.  A non-finite score is MRK_ERR_INVALID_ARG. */
int mrk_train_gradients(mrk_ctx *ctx, const char *config_json, const double *scores, const double *labels, const int64_t *group_offsets,
                        int64_t n_groups, double *out_g, double *out_h);
/* Step 2 (step 2x when the config says backend "xgboost") for one column of n cells (host only, no context): *n_bounds bounds, copied
 * when cap >= *n_bounds. */
int mrk_train_bins(const char *config_json, const double *column, int64_t n, double *out_bounds, int cap, int *n_bounds);
/* Step 2c for one column of n cells (host only, no context): *n_ids kept category ids in ascending order (the bin of an id is its
 * position), copied when cap >= *n_ids.  Uses max_bin of the config. */
int mrk_train_categories(const char *config_json, const double *column, int64_t n, int32_t *out_ids, int cap, int *n_ids);

#ifdef __cplusplus
}
#endif
#endif /* MRK_H */
