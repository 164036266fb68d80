/*
 * umx.h -- C ABI of the MI355X-native UnMicst inference engine (libumx.so).
 *
 * The reference (HMS-IDAC/UnMicst) has no FFI layer: its hot path sits behind three static methods of a
 * Python namespace-class and one TensorFlow call.  Each entry point below names the reference interface it
 * replaces (file:line relative to the reference tree).  Conventions: every function returns 0 on success and a
 * non-zero umx_status otherwise (no exceptions cross the ABI); umx_last_error() gives the message; the caller
 * owns every buffer it passes; a ctx owns its device memory and stream; one ctx per host thread (a ctx is not
 * thread-safe, the library is re-entrant across ctxs).  "_dev" variants take DEVICE pointers and only enqueue
 * work on the ctx stream (call umx_synchronize); the plain variants take HOST pointers and are synchronous.
 * There is no CPU fallback: every compute entry point fails with UMX_ERR_NO_DEVICE without a gfx950 GPU.
 */
#ifndef UMX_H
#define UMX_H

#include <stddef.h>
#include <stdint.h>

#if defined(__GNUC__)
#define UMX_API __attribute__((visibility("default")))
#else
#define UMX_API
#endif

#ifdef __cplusplus
extern "C" {
#endif

typedef struct umx_ctx umx_ctx;

enum umx_status {
    UMX_OK = 0,
    UMX_ERR_INVALID = 1,     /* bad argument / unsupported hyper-parameters */
    UMX_ERR_BLOB = 2,        /* weight blob size does not match the graph (reference: tf NotFoundError on restore) */
    UMX_ERR_NO_DEVICE = 3,   /* no usable HIP device */
    UMX_ERR_HIP = 4,         /* a HIP runtime call failed */
    UMX_ERR_OOM = 5,
    UMX_ERR_RANGE = 6,       /* split-precision path: an activation left the binary16 range (|v| >= 6e4); umx_labeler_run_hmax: a
                              * reconstruction was still rising after UMX_HMAX_MAX_LAUNCHES launches */
    UMX_ERR_GUARD = 7        /* debug guard mode only (UMX_DEBUG_GUARD, umx_create_opts / include/umx_train.h): a kernel wrote outside its buffer */
};

/* Arithmetic of the convolutions.  All hold the 1e-4 tolerance on the probability maps.
 *   UMX_PREC_F32    exact fp32 products on v_mfma_f32_16x16x4_f32 (bit-for-bit an fp32 fma chain).
 *   UMX_PREC_F16X3  every fp32 product as three binary16 MFMA products of a (hi, lo) split of both operands with fp32
 *                   accumulation (~2^-21 relative error per product; 16/3 of the fp32 matrix rate).
 *   UMX_PREC_F16X3_F6  UMX_PREC_F16X3 with the two CROSS terms (x_hi*w_lo + x_lo*w_hi, a 2^-11 correction) of the wide plain
 *                   convolutions at <= 1/4 of the input resolution (>= 2 blocks of 144 output channels: the duo widths' ld3 / ld4 /
 *                   lu3 / lu4 convolutions; no layer of the solo or legacy models) on the block-scaled matrix instruction (OCP MX fp6
 *                   e2m3, 4 x the K per instruction): half the matrix time on those layers, 5 - 13 % of their run time.  1e-6 .. 3e-6
 *                   on the GPU against the oracle, 2e-5 in emulation on the reference's trained weights
 *                   (tests/fp8_cross_term_report.py); every other layer as UMX_PREC_F16X3.
 *   UMX_PREC_DEFAULT  = UMX_PREC_F16X3_F6 where the split-precision planner covers every layer of the graph, else UMX_PREC_F32
 *                   (layers of 4x4 pixels under 7x7 filters exceed the split kernels' halo image) -- said through
 *                   umx_last_error(ctx); UMX_PRECISION=f32|f16x3|f16f6 in the environment pins it.  umx_precision_of() tells
 *                   which one a ctx runs (UMX_PREC_F16X3 when no layer of the model takes the fp6 form). */
enum umx_precision { UMX_PREC_DEFAULT = 0, UMX_PREC_F32 = 1, UMX_PREC_F16X3 = 2, UMX_PREC_F16X3_F6 = 3 };

typedef struct umx_options {
    int32_t device_ordinal;
    int32_t max_batch;       /* tiles per UNet launch group */
    int32_t precision;       /* enum umx_precision */
    int32_t act_shift;       /* F16X3: activations stored times 2^act_shift (0..8); -1 = default (0) */
    int32_t lanes;           /* 0 = default (1), 1 or 2: activation-buffer sets / streams the tile batches of one call
                                alternate between (2: the kernels of consecutive batches overlap; twice the arena) */
    int32_t reserved[11];    /* must be zero */
} umx_options;

enum umx_graph {
    UMX_GRAPH_LEGACY = 0,    /* reference UnMicst.py:51-187 (ReLU, 1x1 shortcut, BN after ReLU, no BN elsewhere) */
    UMX_GRAPH_V2 = 1         /* reference UnMicst1-5.py:55-237 == UnMicst2.py:52-235 at inference */
};

/* The reference's hp dict (UnMicst1-5.py:57-67) + which graph builder consumes it.  downSampFact is fixed at 2. */
typedef struct umx_hparams {
    int32_t graph, imSize, nChannels, nClasses, nOut0, nLayers, ks, nExtraConvs, featMapsFact;
} umx_hparams;

enum umx_mode { UMX_MODE_ACCUMULATE = 0, UMX_MODE_REPLACE = 1 };      /* PI2D.Mode, PartitionOfImage.py:75 */
enum umx_stitch { UMX_STITCH_FP16_COMPAT = 0, UMX_STITCH_FP32 = 1 }; /* fp16-compat reproduces the reference's
    float16 Output/Count accumulators bit for bit (PartitionOfImage.py:84-122); fp32 blends in double and
    returns float32 */

/*
 * Weight blob: one flat little-endian float32 array of the raw TensorFlow tensors in graph-execution order
 * (unmicst_amd/model.py: tensor_specs):
 *   for i in 0..nLayers-1:  ld{i}: w1 [ks,ks,Cin,Cout]; nExtraConvs x wextra [ks,ks,Cout,Cout];
 *                           wshort [s,s,Cin,Cout] (s = 1 legacy, ks v2); BN gamma,beta,moving_mean,moving_var [Cout]
 *   lb: w [ks,ks,Cn,2Cn]; (v2 only) BN x4 [2Cn]
 *   for i in nLayers-1..0:  lu{i}: wt [ks,ks,C(i+1),C(i+2)] (conv2d_transpose filter, OUTPUT channel first);
 *                           w2 [ks,ks,C(i)+C(i+1),C(i+1)]; (v2 only) BN x4; nExtraConvs x wextra
 *   lt: w [1,1,C1,nClasses]; (v2 only) BN x4 [nClasses]
 * All folding/packing happens inside umx_create.
 */

/* Replaces the nvidia-smi / NVML device probing of reference UnMicst1-5.py:750-769, toolbox/GPUselect.py:4-22. */
UMX_API int umx_device_count(void);

/* Free / total HBM bytes of one device -- what toolbox/GPUselect.py:4-22 (pick_gpu_lowest_memory, via NVML) reads to
 * choose a device when --GPU is not given (UnMicst1-5.py:751-754).  Either pointer may be NULL. */
UMX_API int umx_device_mem_info(int device_ordinal, size_t* free_bytes, size_t* total_bytes);

/* Replaces UNet2D.singleImageInferenceSetup's graph build + Saver.restore (UnMicst1-5.py:656-682).
 * max_batch = tiles per UNet launch group (activation arena is sized for it; any n is accepted later). */
UMX_API int umx_create(const umx_hparams* hp, const float* weight_blob, size_t blob_floats, int device_ordinal,
               int max_batch, umx_ctx** out);

/* umx_create with explicit options (precision, ...). */
UMX_API int umx_create_opts(const umx_hparams* hp, const float* weight_blob, size_t blob_floats, const umx_options* opts,
                    umx_ctx** out);
/* Debug guard mode.  UMX_DEBUG_GUARD=<byte> (e.g. 0xff), read by umx_create_opts (on every attempt of the default-precision
 * cascade; not a byte: UMX_ERR_INVALID), gives every device buffer of that context -- the create-time ones, the ones the entries
 * grow on demand, the host slots' and a sharded context's -- a red zone of max(64 KiB, its size rounded up to 4 KiB) on both sides,
 * filled with that byte.  Resident buffers (weights, epilogue constants, stage lists, head fragments, the zero line, the range
 * flags) are uploaded or cleared at create.  Every other buffer is call-scoped: it is filled with the byte at allocation and again
 * at the start of every entry that enqueues work, before that entry's first copy or launch, so a result that depends on the byte
 * read memory that THIS call did not write -- a repeated call cannot lean on the previous call's results.  Every such entry
 * (umx_forward_tiles[_dev], umx_band_tiles_dev, umx_stitch_dev, umx_infer_image*, the sharded entries) and umx_synchronize then
 * waits for every stream of the context and checks every zone at its end, umx_infer_image_wait for a submitted call:
 * UMX_ERR_GUARD names the buffer, the side and the first and last changed byte (umx_last_error).  Between calls the mode waits for
 * idle streams, and a submit waits for the other slot; inside one call the launches, streams and events are the normal ones.
 * The umx_test_*_dev entries put their scratch in a call-local arena of the same kind.  Slow; for tests
 * (tests/test_gpu_infer_guard.py).  Off (unset or empty), allocations and launches are exactly the normal ones. */
/* The precision a ctx actually runs (enum umx_precision). */
UMX_API int umx_precision_of(const umx_ctx* ctx);

/* Replaces UNet2D.singleImageInferenceCleanup (UnMicst1-5.py:684-685). NULL is a no-op. */
UMX_API void umx_destroy(umx_ctx* ctx);

/* Message of the last failure on this ctx (ctx == NULL: last failure of a ctx-less call on this thread). */
UMX_API const char* umx_last_error(const umx_ctx* ctx);

/* Use the caller's HIP stream (hipStream_t passed as void*; NULL restores the ctx's own stream). */
UMX_API int umx_set_stream(umx_ctx* ctx, void* hip_stream);
UMX_API int umx_synchronize(umx_ctx* ctx);

/* Replaces Session.run(UNet2D.nn, {tfData: tiles, tfTraining: 0}) (UnMicst1-5.py:704):
 * tiles [n,imSize,imSize,nChannels] float32 NHWC (already normalised) -> probs [n,imSize,imSize,nClasses]. */
UMX_API int umx_forward_tiles(umx_ctx* ctx, const float* tiles_host, int n, float* probs_host);
UMX_API int umx_forward_tiles_dev(umx_ctx* ctx, const float* tiles_dev, int n, float* probs_dev);

/* Tile grid of an H x W image for this model (PI2D.setup, PartitionOfImage.py:23-75; margin = imSize/8,
 * UnMicst1-5.py:694).  Any output pointer may be NULL. */
UMX_API int umx_tile_grid(const umx_ctx* ctx, int H, int W, int* patch_rows, int* patch_cols, int* padded_rows,
                  int* padded_cols);

/* Replaces UNet2D.singleImageInference (UnMicst1-5.py:687-710, UnMicst2.py:666-689, UnMicst.py:520-541) for
 * ALL classes in one pass: image float64 [C_img,H,W] (C_img == 1: the plane is copied to every input channel,
 * as solo does; else C_img == nChannels), already resized/rescaled by the driver.
 * out: [nClasses,H,W], uint16-encoded IEEE float16 for UMX_STITCH_FP16_COMPAT, float32 for UMX_STITCH_FP32. */
UMX_API int umx_infer_image(umx_ctx* ctx, const double* image_host, int C_img, int H, int W, double mean, double std,
                    int mode, int stitch, void* out_host);
UMX_API int umx_infer_image_dev(umx_ctx* ctx, const double* image_dev, int C_img, int H, int W, double mean, double std,
                        int mode, int stitch, void* out_dev);

/* The drivers' whole pre/post-processing around singleImageInference at --scalingFactor 1 and --outlier -1 (reference
 * UnMicst1-5.py:807-821 and :848-854; UnMicst2.py:771-788,813-817; UnMicst.py:618-633,654-656), fused with the path:
 *   raw [C_img,H,W] uint8 (bits 8) or uint16 (bits 16)  ->  float64 in [0,1] (skimage's resize at the identity grid:
 *   multiply by 1/255 or 1/65535)  ->  rescale != 0: rescale_intensity(in (min,max) of the plane, out (0, 0.983)) per
 *   plane (legacy / duo / cyto feed this; solo feeds the un-rescaled plane, rescale == 0)  ->  umx_infer_image (fp16-compat
 *   stitch)  ->  uint8(255 * pm) -> resize (identity) -> uint8(255 * .): out [nClasses,H,W] uint8.
 * Bit-identical to the host-side recipe (unmicst_amd/driver.py); saves the float64 upload and the fp16 download.  With rescale the
 * call finds each plane's (min, max) with host threads (umx_plane_range) while the rows are on their way up, and the tile gather
 * applies the rescale to the raw samples: no pass over the slide precedes the first tile. */
UMX_API int umx_infer_image_raw(umx_ctx* ctx, const void* raw_host, int bits, int C_img, int H, int W, int rescale,
                        double mean, double std, int mode, uint8_t* out_host);

/* umx_infer_image_raw with rescale != 0 and the planes' extrema handed in: range[2 * c], range[2 * c + 1] = (min, max) of plane c's
 * raw samples, as the file reader that produced raw_host found them (the reference's drivers read the page with tifffile and call
 * np.min / np.max on it, UnMicst1-5.py:817-821; UnMicst.py:606-610).  The call then needs no pass over the whole slide in front of its
 * first tile: rows go up and planes come down under the tile kernels, as without a rescale.  The values are trusted (they must be
 * the true extrema for the result to equal umx_infer_image_raw's); range == NULL is umx_infer_image_raw(rescale = 1). */
UMX_API int umx_infer_image_raw_range(umx_ctx* ctx, const void* raw_host, int bits, int C_img, int H, int W, const uint32_t* range,
                                      double mean, double std, int mode, uint8_t* out_host);

/* (min, max) of n uint8 / uint16 samples on the host, one pass on up to 16 threads: the pair umx_infer_image_raw_range takes, for a
 * caller whose reader did not keep it (the reference: np.min / np.max over the page, UnMicst1-5.py:817-821).  No context, no GPU. */
UMX_API int umx_plane_range(const void* raw_host, int bits, size_t n, uint32_t* range);

/* The same recipe at --scalingFactor != 1 (reference UnMicst1-5.py:813-816: resize to (int(H*sf), int(W*sf)) before the
 * inference, :850: resize of the uint8 planes back to (H, W)), with skimage.transform.resize's defaults -- order 1, mode
 * 'reflect', anti-aliasing Gaussian on shrinking axes, clip to the input range -- evaluated in float64 on the device.
 * rescale != 0: rescale_intensity of the RESIZED plane to (0, 0.983).  scaling == 1 is umx_infer_image_raw. */
UMX_API int umx_infer_image_raw_scaled(umx_ctx* ctx, const void* raw_host, int bits, int C_img, int H, int W, double scaling,
                                       int rescale, double mean, double std, int mode, uint8_t* out_host);

/* The same with the drivers' --outlier percentile (reference UnMicst1-5.py:817-821, UnMicst2.py:780-788, UnMicst.py:606-610):
 * rescale_intensity of the resized plane to (min, np.percentile(plane, outlier)) -> (0, 0.983), values above the percentile
 * clipped.  The percentile is exact: the two order statistics numpy interpolates between are found on the device by radix
 * selection over the float64 plane, the interpolation is numpy's (method 'linear').  outlier in [0, 100]; scaling may be 1. */
UMX_API int umx_infer_image_raw_outlier(umx_ctx* ctx, const void* raw_host, int bits, int C_img, int H, int W, double scaling,
                                        double outlier, double mean, double std, int mode, uint8_t* out_host);

/* How the host entry points move data: the slide goes up and the planes come down in the launch groups of the tile loop,
 * on two copy streams, under the tile kernels of the neighbouring groups (pinned host buffers make these true DMA; pageable
 * ones are staged by HIP and still correct).  A stream of slides -- the drivers' per-file loop, reference
 * UnMicst1-5.py:781-876 run once per file by MCMICRO -- can keep two calls in flight: umx_infer_image_raw_submit enqueues
 * one slide on `slot` (0 or 1; each slot owns its device buffers) and returns at once; umx_infer_image_wait blocks until
 * that slot's planes are in out_host and reports its errors (UMX_ERR_RANGE included).  raw_host / out_host must stay
 * valid until the wait.  umx_infer_image_raw == submit on slot 0 + wait. */
UMX_API int umx_infer_image_raw_submit(umx_ctx* ctx, int slot, const void* raw_host, int bits, int C_img, int H, int W,
                                       int rescale, double mean, double std, int mode, uint8_t* out_host);
UMX_API int umx_infer_image_wait(umx_ctx* ctx, int slot);

/*
 * Whole-slide inference sharded over the GPUs of one node, RCCL over xGMI inside the library (the reference is
 * single-device: UnMicst1-5.py:769).  One process (or thread with its own ctx) per GPU:
 *   rank 0: umx_shard_unique_id(&id); hand the 128 bytes to the other ranks over any channel (file, socket, MPI, ...);
 *   every rank: umx_shard_init(ctx, &id, rank, world)                      -- collective (ncclCommInitRank);
 *               umx_shard_plan(&hp, H, W, rank, world, nslabs, 0, ...)     -- which image rows this rank must hold;
 *               umx_infer_image_sharded_dev(ctx, band_dev, ...)            -- collective; every rank ends up with the full
 *                                                                             [nClasses,H,W] result in out_full_dev;
 *               umx_synchronize(ctx); ... ; umx_shard_fini(ctx) (or umx_destroy).
 * Patch rows are split into contiguous bands; a rank computes the tiles of its band from the image rows [need_row0,
 * need_row1) it holds (band_dev = those rows, float64 [C_img, band_rows, W], band_row0 = first row held), sends the
 * probabilities of its last patch row to the next rank, stitches the rows it owns -- visiting tiles in ascending global
 * index, so the fp16 result is bit-identical to a one-GPU run -- and all-gathers them slab by slab under the tiles of
 * the next slab.  RCCL is resolved at run time (dlopen of the librccl the process already holds, else ROCm's;
 * UMX_RCCL_PATH overrides).  unmicst_amd/sharding.py is the same schedule over torch.distributed.
 */
typedef struct umx_unique_id { char internal[128]; } umx_unique_id;   /* == ncclUniqueId */
UMX_API int umx_shard_unique_id(umx_unique_id* out);
UMX_API int umx_shard_init(umx_ctx* ctx, const umx_unique_id* id, int rank, int world);
/* The inter-rank operations of the schedule as a table: umx_shard_init fills it with RCCL; umx_shard_init_transport takes the
 * caller's instead (MPI, sockets, a host-staged stand-in -- how tests/test_gpu_parity.py runs the band / halo / scatter code of
 * umx_infer_image_sharded_dev in worlds of 2 and 3 on one GPU, where RCCL refuses to put two ranks on a device).  Semantics are
 * RCCL's: `stream` is a hipStream_t; an operation takes effect in stream order (a blocking implementation synchronises the stream,
 * moves the bytes and returns); send / recv between group_start and group_end may be matched in any order (either may be NULL);
 * all_gather: every rank contributes bytes_per_rank at send_dev and receives world * bytes_per_rank at recv_dev, rank order;
 * non-zero return = failure (UMX_ERR_HIP).  `peer` is a rank of the world given to the init call. */
typedef struct umx_shard_transport {
    void* user;
    int (*send)(void* user, const void* dev, size_t bytes, int peer, void* stream);
    int (*recv)(void* user, void* dev, size_t bytes, int peer, void* stream);
    int (*all_gather)(void* user, const void* send_dev, void* recv_dev, size_t bytes_per_rank, void* stream);
    int (*group_start)(void* user);
    int (*group_end)(void* user);
} umx_shard_transport;
UMX_API int umx_shard_init_transport(umx_ctx* ctx, const umx_shard_transport* transport, int rank, int world);
UMX_API int umx_shard_fini(umx_ctx* ctx);
/* Geometry of rank `rank` of `world` for an H x W image cut into `nslabs` slabs per band (the count actually used --
 * no more than the smallest band's patch rows -- comes back in nslabs_used): its patch rows, the image rows its tiles read
 * (what band_dev must cover), the image rows it stitches, and the rows of slab `slab`.  Any output may be NULL. */
UMX_API int umx_shard_plan(const umx_hparams* hp, int H, int W, int rank, int world, int nslabs, int slab, int* patch_row0,
                           int* patch_row1, int* need_row0, int* need_row1, int* own_row0, int* own_row1, int* slab_row0,
                           int* slab_row1, int* nslabs_used);
UMX_API int umx_infer_image_sharded_dev(umx_ctx* ctx, const double* band_dev, int C_img, int H, int W, int band_row0,
                                        int band_rows, double mean, double std, int mode, int stitch, int nslabs,
                                        void* out_full_dev);

/* The sharded schedule fed like the one-GPU line (umx_infer_image_raw_submit; SURVEY section 8(e), no reference counterpart:
 * UnMicst1-5.py:769 is single-device).  band_host = this rank's raw uint8 / uint16 rows [C_img, band_rows, W] (image rows
 * [band_row0, band_row0 + band_rows) = need_row0 .. need_row1 of umx_shard_plan), staged piece by piece on the upload stream ahead
 * of the tiles that read them; im2double happens in the tile gather.  range: NULL = no intensity rescale (the solo driver,
 * UnMicst1-5.py:816-821); else the (min, max) of EACH WHOLE plane (2 words per plane, as for umx_infer_image_raw_range -- a rank
 * holds only its band, the caller's reader saw the file) and the gather applies rescale_intensity to (0, 0.983).  Stitched slabs
 * are cast to the drivers' uint8 (UnMicst1-5.py:848-854 at the identity grid) and all-gathered as uint8; every rank ends up with
 * the full [nClasses, H, W] uint8 stack in out_full_dev (NULL: a buffer the library owns), and this rank's own rows
 * [own_row0, own_row1) go down to own_out_host [nClasses, own rows, W] (NULL: no download) on the download stream under the next
 * slab's tiles.  _submit enqueues on `slot` (0 or 1) and returns; umx_infer_image_wait(ctx, slot) completes it (errors,
 * UMX_ERR_RANGE included); band_host / own_out_host / out_full_dev must stay valid until then.  Collective over the world of
 * umx_shard_init.  Bit-identical, row for row, to umx_infer_image_raw[_range] of the whole slide on one GPU. */
UMX_API int umx_infer_image_sharded_raw_submit(umx_ctx* ctx, int slot, const void* band_host, int bits, int C_img, int H, int W,
                                               int band_row0, int band_rows, const uint32_t* range, double mean, double std,
                                               int mode, int nslabs, uint8_t* own_out_host, uint8_t* out_full_dev);
UMX_API int umx_infer_image_sharded_raw(umx_ctx* ctx, const void* band_host, int bits, int C_img, int H, int W, int band_row0,
                                        int band_rows, const uint32_t* range, double mean, double std, int mode, int nslabs,
                                        uint8_t* own_out_host, uint8_t* out_full_dev);

/*
 * Label mask (no reference counterpart: the reference's tools stop at probability maps).  From the stack
 * u8[K][H][W] of final uint8 probability planes in the model's class order, a class c and a minimum area A:
 *   object pixels  pred(y, x) == c, pred = the index of the FIRST maximum of u8[0..K-1][y][x] (a tie goes to the lower class);
 *   objects        their 4-connected components (UMX_BORDER_CONNECTIVITY of include/umx_train.h);
 *   labels         int32 [H][W]: the kept objects (area >= A) numbered 1..N in raster order of their first pixel, 0 elsewhere --
 *                  scipy.ndimage.label with its default structure, the area filter, and a renumbering that keeps the order;
 *   table          one umx_label_object per kept object in label order, integers throughout (centroid = sum / area on the host).
 * Growth (grow_radius R >= 1 and a class set G): the contour class keeps touching nuclei apart
 * and is also the rim of every nucleus, so the objects above are the cores.  With R > 0 the kept objects are seeds (min_area applies
 * to them, before any growth) and grow back over the domain = pixels with label 0 whose pred is in G, in R synchronous levels: at
 * every level each domain pixel that is still 0 and has a labelled 4-neighbour takes the smallest label among them, all pixels
 * deciding on the state of the level before.  N and the numbering do not change; every object keeps its seed and stays
 * 4-connected; a pixel goes to a seed nearest through the domain, a tie to the smaller label; the table is that of the grown labels.
 * Every value is an integer, so nothing depends on the order in which atomics arrive: two calls give the same bytes.
 * A labeler needs no model: it owns a stream and its device buffers (two int32 planes of H * W, the K input planes, one int32 per
 * UMX_LABEL_SCAN_BLOCK pixels and the table; from its first split or flood run on one more int32 plane and one byte plane), grown on demand and
 * kept between runs.  UMX_DEBUG_GUARD (include/umx_train.h) puts red
 * zones round them; a run then ends with their check (UMX_ERR_GUARD).  One labeler per host thread.
 */
typedef struct umx_label_options {
    int32_t cls;             /* 0 .. K-1, in the model's class order */
    int32_t min_area;        /* 1 .. UMX_LABEL_MAX_MIN_AREA pixels */
    int32_t grow_radius;     /* 0: no growth (then grow_classes must be 0 too); else 1 .. UMX_LABEL_MAX_GROW levels */
    uint32_t grow_classes;   /* bit k set: class k (model's class order, k < K) belongs to the growth domain */
    int32_t reserved[4];     /* must be zero */
} umx_label_options;             /* 32 bytes; grow_radius and grow_classes were reserved words: zero is the call of before */
typedef struct umx_label_object {
    int32_t area, y0, x0, y1, x1, reserved;   /* pixels; the inclusive bounding box */
    int64_t sum_y, sum_x;                     /* over the object's pixels */
} umx_label_object;                           /* 40 bytes */
typedef struct umx_labeler umx_labeler;
#define UMX_LABEL_MAX_CLASSES 16
#define UMX_LABEL_MAX_MIN_AREA 65536   /* == UMX_OBJECT_MAX_MIN_AREA */
/* The geometry of the kernels (umx_label.hip), for tests that must cross every boundary of it: rows of the image one workgroup
 * merges in the first merge launch (the seams between such strips are joined pairwise in log2 further launches), threads of a merge
 * workgroup (a seam is walked UMX_LABEL_THREADS pixels at a time), pixels per block of the numbering scan (whose block counts one
 * workgroup scans UMX_LABEL_THREADS at a time). */
#define UMX_LABEL_STRIP_ROWS 32
#define UMX_LABEL_THREADS 1024
#define UMX_LABEL_SCAN_BLOCK 2048
/* The growth: its largest radius, and the geometry of its kernel -- a workgroup owns a tile of UMX_LABEL_GROW_TILE x
 * UMX_LABEL_GROW_TILE pixels and loads UMX_LABEL_GROW_HALO more on every side, so one launch advances up to UMX_LABEL_GROW_HALO
 * levels and a call takes ceil(R / UMX_LABEL_GROW_HALO) of them.  (Enumerators: constant expressions in C and C++ alike.) */
enum { UMX_LABEL_MAX_GROW = 255, UMX_LABEL_GROW_TILE = 64, UMX_LABEL_GROW_HALO = 8 };
/* Host only, no device: H, W >= 1; H * W <= 2^31 - 1 (a flat pixel index is an int32); 1 <= K <= 16; 0 <= cls < K;
 * 1 <= min_area <= 65536; grow_radius 0 with grow_classes 0, or 1 <= grow_radius <= 255 with a non-empty grow_classes that has no
 * bit at or above K; reserved words zero.  UMX_OK, or UMX_ERR_INVALID with the reason in msg (cap bytes; may be NULL). */
UMX_API int umx_label_options_check(const umx_label_options* o, int K, int H, int W, char* msg, size_t cap);
/* UMX_ERR_NO_DEVICE without a gfx950 device: there is no CPU fallback. */
UMX_API int umx_labeler_create(int device_ordinal, umx_labeler** out);
UMX_API void umx_labeler_destroy(umx_labeler* lb);   /* NULL is a no-op */
/* Message of the last failure of this labeler (NULL: of a labeler-less call on this thread). */
UMX_API const char* umx_labeler_last_error(const umx_labeler* lb);
/* Synchronous.  planes_host: uint8 [K][H][W]; labels_host: int32 [H][W], or NULL when only the count and the table are wanted.
 * A refused call (UMX_ERR_INVALID) has touched nothing and leaves the labeler usable. */
UMX_API int umx_labeler_run(umx_labeler* lb, const uint8_t* planes_host, int K, int H, int W, const umx_label_options* o,
                            int32_t* labels_host, int64_t* n_objects);
/* The same on DEVICE pointers of the labeler's device (e.g. the out_full_dev of umx_infer_image_sharded_raw): no upload and no
 * download of the planes.  The planes must be complete when the call is made (the labeler's stream does not wait for the stream that
 * wrote them), and the call returns with the labeler's stream idle: the count comes back to the host in the middle of it. */
UMX_API int umx_labeler_run_dev(umx_labeler* lb, const uint8_t* planes_dev, int K, int H, int W, const umx_label_options* o,
                                int32_t* labels_dev, int64_t* n_objects);
/* The table of the last run: min(cap, N) records into out (may be NULL with cap 0), N into *n. */
UMX_API int umx_labeler_objects(const umx_labeler* lb, umx_label_object* out, int64_t cap, int64_t* n);
/* Milliseconds of the last run by HIP events on the labeler's stream: the upload of the planes, the launches (the read-back of the
 * count in their middle included), the download of the labels and the table.  0 for a part the call did not have.  Any may be NULL. */
UMX_API int umx_labeler_last_ms(const umx_labeler* lb, double* upload_ms, double* kernel_ms, double* download_ms);

/*
 * Intensity of every labelled object in the planes of an image.  From labels int32 [H][W]
 * with values in 0..N and image planes v of type T [C][H][W], T uint8 or uint16, for every plane c and label j = 1..N over the
 * pixels with labels == j:
 *   8. count, sum = the sum of v, sum_sq = the sum of v * v, min, max -- record c * N + (j - 1), plane-major.  A label no pixel
 *      carries gives count 0, sum 0, sum_sq 0, min UINT32_MAX, max 0.  A label value < 0 or > N counts as 0 and is never used as an
 *      index.  sum_sq < 2^31 * 2^32: nothing overflows.
 *   9. mean = sum / count and std = sqrt(max(sum_sq / count - mean * mean, 0)) are host arithmetic in float64, stated here once.
 * Everything is an integer and every atomic an integer add / min / max that nothing reads before its launch ends: two calls give
 * the same bytes.  One launch measures a group of up to UMX_LABEL_MEASURE_GROUP planes with the label plane read once; per row run
 * and plane it costs two 64-bit adds, one 32-bit add, one min and one max at record [c][label - 1].  Known limit, as for the table
 * of the labelling ("salt"): an object made of 10^7 row runs serialises its atomics.
 */
typedef struct umx_label_measure {
    uint64_t sum, sum_sq;
    uint32_t min, max, count, reserved;
} umx_label_measure;   /* 32 bytes */
#define UMX_MEASURE_U8 1
#define UMX_MEASURE_U16 2
/* Planes one launch measures with the label plane read once, and the most planes of one call.  (The values stand in macros of the
 * UMX_MEASURE_ family: the sets of UMX_LABEL_ macros and of UMX_LABEL_ enumerators with a literal value are those of the labelling
 * and of the growth, and tests/test_label_cpu.py and tests/test_label_grow_cpu.py hold them to exactly that.) */
#define UMX_MEASURE_GROUP_PLANES 4
#define UMX_MEASURE_MAX_PLANES 1024
enum { UMX_LABEL_MEASURE_GROUP = UMX_MEASURE_GROUP_PLANES, UMX_LABEL_MAX_MEASURE_PLANES = UMX_MEASURE_MAX_PLANES };
/* Host only, no device: dtype UMX_MEASURE_U8 or _U16; 1 <= C <= 1024; H, W >= 1; H * W <= 2^31 - 1; 0 <= n_objects <= 2^31 - 1 (a
 * label is an int32).  UMX_OK, or UMX_ERR_INVALID with the reason in msg (cap bytes; may be NULL). */
UMX_API int umx_label_measure_check(int dtype, int C, int H, int W, int64_t n_objects, char* msg, size_t cap);
/* planes_host [C][H][W] against the labels of the last successful umx_labeler_run that was given a labels_host: they are still on
 * the device.  The planes go up and are measured group by group; C * N records into out (cap: its records), N into *n (may be NULL).
 * out NULL with cap 0: only N into *n.  UMX_ERR_INVALID -- nothing touched, the labeler usable, the resident labels kept -- when there
 * was no such run, when a later run had no label plane, was umx_labeler_run_dev or failed, when H or W differ from that run's, or
 * when cap < C * N.  A refused run leaves the resident labels as they were.  Synchronous: returns with the stream idle, and under
 * UMX_DEBUG_GUARD ends in the check of the red zones. */
UMX_API int umx_labeler_measure(umx_labeler* lb, const void* planes_host, int dtype, int C, int H, int W, umx_label_measure* out,
                                int64_t cap, int64_t* n);
/* The same on DEVICE pointers of the labeler's device: labels_dev int32 [H][W] with objects 1..n_objects, planes_dev [C][H][W],
 * both complete when the call is made and only read.  Needs no prior run and leaves the resident labels alone.  C * n_objects
 * records into out_host (cap >= that).  Synchronous, guard check as above. */
UMX_API int umx_labeler_measure_dev(umx_labeler* lb, const int32_t* labels_dev, int64_t n_objects, const void* planes_dev, int dtype,
                                    int C, int H, int W, umx_label_measure* out_host, int64_t cap);
/* Milliseconds of the last measurement, summed over its groups: the uploads of the planes (0 for _dev), the launches, the downloads
 * of the records.  Any may be NULL. */
UMX_API int umx_labeler_measure_last_ms(const umx_labeler* lb, double* upload_ms, double* kernel_ms, double* download_ms);

/*
 * Shape of every labelled object (the definition is the project's own).  From labels int32
 * [H][W] with objects 1..N -- a value < 0 or > N counts as 0 and is never used as an index; a label need not be connected -- for
 * every label j, with M_j the mask labels == j padded with one ring of 0:
 *   16. one umx_label_shape, record j - 1: the sums of y, x, y * y, y * x and x * x over the pixels of M_j in image coordinates, and
 *       the numbers of the (H + 1) x (W + 1) 2x2 windows of the padded mask that hold exactly one pixel of M_j (q1), two that share
 *       an edge (q2), two on a diagonal (qd), three (q3), four (q4).  A window is classified per label: one with pixels of two labels
 *       counts once for each, by that label's own pattern.  A label no pixel carries gives all zeros.
 *   17. 4 * area = q1 + 2 q2 + 2 qd + 3 q3 + 4 q4;  edges = q1 + q2 + 2 qd + q3 is the number of pixel edges between M_j and its
 *       complement, the image border included;  euler = (q1 - q3 + 2 qd) / 4 divides exactly and is the Euler number for a
 *       4-connected foreground and an 8-connected background; for a 4-connected object holes = 1 - euler.
 *   18. axes, eccentricity, orientation and the perimeter estimate are host arithmetic in float64 on these integers, stated once in
 *       unmicst_amd/umx.py shape_descriptors (DESIGN.md has the formulas).
 * Limits: 1 <= H, W <= 65536, H * W <= 2^31 - 1, 0 <= n_objects <= 2^31 - 1.  Then y * y and x * x are below 2^32 and area below
 * 2^31, so every sum stays below 2^63; a window count is at most (H + 1) * (W + 1) <= 2^31 + 2^17 + 1 < 2^32.
 * Everything is an integer and every atomic an integer add that nothing reads before its launch ends: two calls give the same
 * bytes.  One launch, one wave per row; per row run at most five 64-bit adds and five 32-bit ones (an addend of 0 is skipped; a run
 * inside an object has only q4) at record label - 1.  Known limit, as for the measurement ("salt"): an object made of 10^7 row runs
 * serialises its atomics.
 */
typedef struct umx_label_shape {
    int64_t sum_y, sum_x, sum_yy, sum_xy, sum_xx;
    uint32_t q1, q2, qd, q3, q4, reserved;
} umx_label_shape;   /* 64 bytes */
/* The largest side of a plane whose shapes are taken: the squares of its coordinates stay below 2^32. */
#define UMX_SHAPE_MAX_SIDE 65536
/* Host only, no device: 1 <= H, W <= 65536; H * W <= 2^31 - 1; 0 <= n_objects <= 2^31 - 1.  UMX_OK, or UMX_ERR_INVALID with the
 * reason in msg (cap bytes; may be NULL). */
UMX_API int umx_label_shape_check(int H, int W, int64_t n_objects, char* msg, size_t cap);
/* The shapes of the labels of the last successful host run that was given a label plane (plain, grown or split): they are still on
 * the device.  N records into out (cap: its records), N into *n (may be NULL); out NULL with cap 0: only N into *n.  Refusals as
 * umx_labeler_measure's (UMX_ERR_INVALID, nothing touched, the labeler usable, the resident labels kept): no such run, a later run
 * without a label plane or on device pointers or a failed one, H or W other than that run's, cap < N.  Synchronous: returns with
 * the stream idle, and under UMX_DEBUG_GUARD ends in the check of the red zones.  The records live in the labeler's arena, grown on
 * demand and kept. */
UMX_API int umx_labeler_shape(umx_labeler* lb, int H, int W, umx_label_shape* out, int64_t cap, int64_t* n);
/* The same on a DEVICE pointer of the labeler's device: labels_dev int32 [H][W] with objects 1..n_objects, complete when the call is
 * made and only read.  Needs no prior run and leaves the resident labels alone.  n_objects records into out_host (cap >= that). */
UMX_API int umx_labeler_shape_dev(umx_labeler* lb, const int32_t* labels_dev, int64_t n_objects, int H, int W, umx_label_shape* out_host,
                                  int64_t cap);
/* Milliseconds of the last shape call: the two launches, the download of the records.  Either may be NULL. */
UMX_API int umx_labeler_shape_last_ms(const umx_labeler* lb, double* kernel_ms, double* download_ms);

/*
 * Which labelled objects touch, and along how many pixel edges (the definition is the
 * project's own).  From labels int32 [H][W] with objects 1..N -- a value < 0 or > N counts as 0 and is never used as an index:
 *   22. contacts: a pixel edge is a pair of horizontally or vertically adjacent pixels, both inside the image (diagonal neighbours
 *       do not count: UMX_BORDER_CONNECTIVITY).  For labels a < b, edges(a, b) is the number of pixel edges whose two pixels carry a
 *       and b, in either order; the pair is a contact iff edges > 0.  One umx_label_contact per contact, sorted by (a, b) ascending;
 *       M is their number.  edges <= 2 H W < 2^32.
 *   23. reach R, 1 .. UMX_CONTACT_MAX_REACH: the contacts are taken from a scratch plane S instead -- the labels (values outside 1..N
 *       as 0) grown R levels by the growth rule of umx_labeler_run's step 6 over the domain "label 0", no class consulted.  Two
 *       objects with a gap between them are then neighbours when their fronts meet within R levels and no third object lies
 *       between.  S is scratch: the labels, the object table and what the measurement and the shapes see are bit for bit what they
 *       were.  R = 0 is step 22 on the labels themselves.
 *   24. the degree of an object (the contacts it takes part in) and its total shared edges are host arithmetic on the list, stated
 *       once in unmicst_amd/umx.py contact_degrees.
 * After a plain run the list is empty (4-connected components of one class never touch); after a growth, a split or a flood it
 * is the set of cut lines those steps drew.  Everything is an integer and the list a set with counts in canonical order: two calls
 * give the same bytes, in whatever order threads and atomics run.
 * The device side: one pass over the plane (one wave per row; equal pairs on consecutive pixels collapse to one insertion) into an
 * open-addressing table of UMX_CONTACT_TABLE_MIN entries or the power of two at or above n_objects, whichever is larger, of 12
 * bytes each; a pass that finds no slot within UMX_CONTACT_PROBE_MAX probes is run again with the table doubled, and beyond
 * UMX_CONTACT_TABLE_MAX entries the call is refused with a message (UMX_ERR_OOM).  The list is ordered on the device when no object has more
 * than UMX_CONTACT_DEVICE_SORT_MAX contacts (a rank by counting inside each object's row), else on the host; both give the same
 * bytes.  A reach of R needs one scratch plane of H * W int32, two when R > 8: the labeler's second plane and the split's third one
 * where a run has allocated them large enough, else allocations of their own, kept like the others.
 */
typedef struct umx_label_contact {
    int32_t a, b;            /* the two labels, 1 <= a < b <= N */
    uint32_t edges;          /* pixel edges between them, >= 1 */
    uint32_t reserved;       /* 0 */
} umx_label_contact;         /* 16 bytes */
typedef struct umx_label_contact_stats {
    int64_t table_capacity;  /* entries of the table of the last pass */
    int64_t reruns;          /* passes of the last call that found the table too small and were run again */
    int64_t longest_row;     /* the largest number of contacts (a, .) of one label a: what the ordering is chosen by */
    int32_t ordered_by;      /* who ordered the list: one of the three codes below */
    int32_t reserved;
} umx_label_contact_stats;   /* 32 bytes */
#define UMX_CONTACT_MAX_REACH 255
#define UMX_CONTACT_TABLE_MIN 65536
#define UMX_CONTACT_TABLE_MAX 268435456
#define UMX_CONTACT_PROBE_MAX 1024
#define UMX_CONTACT_DEVICE_SORT_MAX 1024
/* ordered_by: nothing to order (M == 0, or only M was asked for) | the device | the host (a row longer than the cap above) */
#define UMX_CONTACT_ORDER_NONE 0
#define UMX_CONTACT_ORDER_DEVICE 1
#define UMX_CONTACT_ORDER_HOST 2
/* Host only, no device: H, W >= 1; H * W <= 2^31 - 1; 0 <= n_objects <= 2^31 - 1; 0 <= reach <= 255.  UMX_OK, or UMX_ERR_INVALID
 * with the reason in msg (cap bytes; may be NULL). */
UMX_API int umx_label_contact_check(int H, int W, int64_t n_objects, int reach, char* msg, size_t cap);
/* The contacts of the labels of the last successful host run that was given a label plane (plain, grown, split or flooded): they
 * are still on the device.  M records into out (cap: its records), M into *m (may be NULL); out NULL with cap 0: only M into *m.
 * Refusals as umx_labeler_shape's (UMX_ERR_INVALID, nothing touched, the labeler usable, the resident labels kept): no such run, a
 * later run without a label plane or on device pointers or a failed one, H or W other than that run's, a reach outside 0..255; and
 * cap < M, with M stored in *m (M is known only after the pass: the device has worked, out is untouched).  Synchronous: returns with
 * the stream idle, and under UMX_DEBUG_GUARD ends in the check of the red zones.  All device memory is the labeler's arena's, grown
 * on demand and kept. */
UMX_API int umx_labeler_contacts(umx_labeler* lb, int H, int W, int reach, umx_label_contact* out, int64_t cap, int64_t* m);
/* The same on a DEVICE pointer of the labeler's device: labels_dev int32 [H][W] with objects 1..n_objects, complete when the call is
 * made and only read.  Needs no prior run and leaves the resident labels alone. */
UMX_API int umx_labeler_contacts_dev(umx_labeler* lb, const int32_t* labels_dev, int64_t n_objects, int H, int W, int reach,
                                     umx_label_contact* out_host, int64_t cap, int64_t* m);
/* Milliseconds of the last contacts call: its launches (every pass, the growth of a reach and the ordering), the download of the
 * records.  Either may be NULL. */
UMX_API int umx_labeler_contacts_last_ms(const umx_labeler* lb, double* kernel_ms, double* download_ms);
/* How the last contacts call went.  UMX_ERR_INVALID for a null argument. */
UMX_API int umx_labeler_contacts_last_stats(const umx_labeler* lb, umx_label_contact_stats* stats);

/*
 * The convex hull of every labelled object, and with it solidity and the Feret diameters (the
 * definition is the project's own).  From labels int32 [H][W] with objects 1..N -- a value < 0 or > N counts as 0 and is never used
 * as an index; a label need not be connected and need not occur.  Pixel (y, x) is the closed unit square [y, y + 1] x [x, x + 1];
 * its four corners are lattice points with 0 <= y <= H and 0 <= x <= W, and every coordinate below is on that corner lattice.
 *   25. hull(j) is the convex hull of the squares of all pixels with label j.  It is never degenerate: one pixel gives the unit
 *       square.  Its vertices are the strictly convex corners only (collinear points are dropped), listed from the vertex with the
 *       smallest (y, x) in the direction in which sum_i (x_i * y_{i+1} - x_{i+1} * y_i) is positive: the second vertex is the other
 *       end of the top edge, with the same y and a larger x.
 *   26. one umx_label_hull per label, record j - 1.  A label no pixel carries gives zeros in every field but `first`, which is the
 *       running offset: first[j] = the sum of n_vertices of all labels below j, for every record.
 *   27. the vertex list: all hulls one after the other in label order, V umx_label_hull_vertex in all.
 *   28. hull area, solidity (area over hull area), the Feret diameters and the hull's perimeter are host arithmetic in float64 on
 *       these integers, stated once in unmicst_amd/umx.py hull_descriptors (DESIGN.md has the formulas).
 * Limits: 1 <= H, W <= 65536, H * W <= 2^31 - 1, 0 <= n_objects <= 2^31 - 1.  Then a coordinate is at most 2^16, a squared distance
 * at most 2^33, every cross-product term at most 2^32 (formed in 64 bits) and area2 at most 2^32.  A second limit is known only after
 * the first pass: E, the sum over the labels of ymax - ymin + 1 (the rows of their boxes), is at most the number of object pixels
 * for 4-connected objects but reaches N * H for labels in far-apart pieces; above UMX_HULL_MAX_ROWS the call is refused with
 * UMX_ERR_OOM and a message, before anything is allocated for it, and the resident labels are kept.
 * Everything is an integer and both lists are canonical: two calls give the same bytes, in whatever order threads and atomics run.
 * The device side: one wave per row for each label's row range (atomicMin / atomicMax of y per row run), a 64-bit prefix sum of the
 * heights (E comes back to the host), one wave per row again for the least x and the largest x + 1 of each label in each row of its
 * box (8 bytes a row), one wave per object for the hull (a gift wrap by wave reductions on 64-bit cross products, down the right
 * chain and up the left one; the vertices into a scratch area of 2 * rows + 2 places an object, a bound that is attained), a
 * prefix sum of the vertex counts (V comes back) and one wave per object again to compact the vertices into the list.
 */
typedef struct umx_label_hull {
    int64_t area2;           /* twice the hull's area: the shoelace sum of step 25, an integer */
    int64_t feret_max_sq;    /* the largest squared distance between two hull vertices */
    int64_t first;           /* index of the label's first vertex in the vertex list */
    int32_t n_vertices;      /* hull vertices, 0 or >= 4 */
    int32_t rows;            /* image rows in which the label has at least one pixel */
} umx_label_hull;            /* 32 bytes */
typedef struct umx_label_hull_vertex {
    int32_t y, x;            /* a corner: 0 <= y <= H, 0 <= x <= W */
} umx_label_hull_vertex;     /* 8 bytes */
/* The largest side of a plane whose hulls are taken, and the largest E (above). */
#define UMX_HULL_MAX_SIDE 65536
#define UMX_HULL_MAX_ROWS 268435456
/* Host only, no device: 1 <= H, W <= 65536; H * W <= 2^31 - 1; 0 <= n_objects <= 2^31 - 1.  UMX_OK, or UMX_ERR_INVALID with the
 * reason in msg (cap bytes; may be NULL). */
UMX_API int umx_label_hull_check(int H, int W, int64_t n_objects, char* msg, size_t cap);
/* The hulls of the labels of the last successful host run that was given a label plane (plain, grown, split or flooded): they are
 * still on the device.  N records into out (cap: its records) and N into *n, V vertices into verts (vcap: its entries) and V into
 * *v; n and v may be NULL.  out NULL with cap 0 and verts NULL with vcap 0: only N and V.  Refusals as umx_labeler_shape's
 * (UMX_ERR_INVALID, nothing touched, the labeler usable, the resident labels kept): no such run, a later run without a label plane
 * or on device pointers or a failed one, H or W other than that run's, cap < N; and vcap < V, with V stored in *v (V is known only
 * after the passes: the device has worked, out and verts are untouched); and E > UMX_HULL_MAX_ROWS (UMX_ERR_OOM).  Synchronous:
 * returns with the stream idle, and under UMX_DEBUG_GUARD ends in the check of the red zones.  All device memory is the labeler's
 * arena's, grown on demand and kept. */
UMX_API int umx_labeler_hull(umx_labeler* lb, int H, int W, umx_label_hull* out, int64_t cap, int64_t* n, umx_label_hull_vertex* verts,
                             int64_t vcap, int64_t* v);
/* The same on a DEVICE pointer of the labeler's device: labels_dev int32 [H][W] with objects 1..n_objects, complete when the call is
 * made and only read.  Needs no prior run and leaves the resident labels alone.  n_objects records into out_host (cap >= that). */
UMX_API int umx_labeler_hull_dev(umx_labeler* lb, const int32_t* labels_dev, int64_t n_objects, int H, int W, umx_label_hull* out_host,
                                 int64_t cap, umx_label_hull_vertex* verts_host, int64_t vcap, int64_t* v);
/* Milliseconds of the last hull call: its launches (the two host synchronisations for E and V among them), the download of the
 * records and the vertices.  Either may be NULL. */
UMX_API int umx_labeler_hull_last_ms(const umx_labeler* lb, double* kernel_ms, double* download_ms);

/*
 * Relabel: drop some objects, merge others, renumber the rest 1..N' without a gap (the
 * definition is the project's own).  From labels int32 [H][W] with values in 0..N, keep (N bytes, keep[j - 1] != 0 keeps label j; NULL
 * keeps all) and M pairs of int32 labels (a, b):
 *   29. classes: the equivalence closure of the pairs on 1..N.  a == b, repeated pairs and (b, a) change nothing; pairs need not
 *       touch (a merged object may be disconnected).  A pair that names a label outside 1..N, or a label that keep drops, is
 *       refused, and the message gives the pair's index: a label is dropped or merged, never both.
 *   30. numbering: a class is kept iff its members are (by 29 it is wholly kept or one dropped label); the kept classes are
 *       numbered 1..N' in order of their least member; map[0] = 0 and map[j] = the number of j's class, 0 when j is dropped.  The
 *       order of the least members is kept, so labels in raster order of their first pixel stay so.
 *   31. labels'(y, x) = map[labels(y, x)]; a value < 0 or > N counts as 0 and is never used as an index (the rule of step 8).
 *   32. the umx_label_object of a new label is the merge of its members' records: area, sum_y, sum_x added, y0 and x0 by minimum,
 *       y1 and x1 by maximum -- what step 4 gives on labels'.
 * Everything is an integer: two calls give the same bytes, whatever the order of the pairs.  keep all with no pair is the identity;
 * relabel(k2) after relabel(k1) is relabel(k1 & k2[map1]).
 * Steps 29 and 30 run on the host (a union-find with path compression over the N + 1 words of map), 31 and 32 on the device: the map
 * is uploaded into an allocation of its own (4 (N + 1) bytes), the new table is a second table buffer that changes places with the
 * first, and the plane pass looks the map up once per row run, not per pixel.
 */
#define UMX_RELABEL_MAX_PAIRS 268435456   /* == UMX_CONTACT_TABLE_MAX: the pairs come from a contacts list */
/* Host only, no device: H, W >= 1; H * W <= 2^31 - 1; 0 <= n_objects <= 2^31 - 2 (the map has n_objects + 1 int32 words);
 * 0 <= n_pairs <= UMX_RELABEL_MAX_PAIRS.  UMX_OK, or UMX_ERR_INVALID with the reason in msg (cap bytes; may be NULL). */
UMX_API int umx_label_relabel_check(int H, int W, int64_t n_objects, int64_t n_pairs, char* msg, size_t cap);
/* Steps 29 and 30, host only, no device: map (n_objects + 1 words) and *n_new = N'.  keep: n_objects bytes, or NULL for all; pairs:
 * 2 * n_pairs words.  map NULL: the arguments are only validated and *n_new is not written.  UMX_OK, or UMX_ERR_INVALID with the
 * reason in msg (a refused call may have written map). */
UMX_API int umx_label_relabel_map(int64_t n_objects, const uint8_t* keep /* NULL: all */, const int32_t* pairs, int64_t n_pairs,
                                  int32_t* map /* n_objects + 1 */, int64_t* n_new, char* msg, size_t cap);
/* On the resident labels (those of the last umx_labeler_run that was given a label plane): edits the label plane and the object
 * table on the device in place and sets their count to N'; labels_host (may be NULL) receives the new plane, map_host (may be NULL;
 * N + 1 words) the map.  keep == NULL goes with n_keep == 0; else n_keep must be N.  Synchronous.  Refused (UMX_ERR_INVALID) before
 * any device work, with the labels, the table and the labeler as they were: no valid resident labels, another H or W, n_keep != N, a
 * bad pair.  A HIP failure after the first launch leaves the labeler without resident labels.  Afterwards umx_labeler_objects,
 * _measure, _shape, _contacts and _hull see the new labels and N'; the counts of a split or a flood stay those of the run. */
UMX_API int umx_labeler_relabel(umx_labeler* lb, int H, int W, const uint8_t* keep, int64_t n_keep, const int32_t* pairs, int64_t n_pairs,
                                int32_t* labels_host, int32_t* map_host /* may be NULL; N + 1 */, int64_t* n_new);
/* The same on the caller's DEVICE plane with objects 1..n_objects, complete when the call is made; labels_out_dev may equal
 * labels_dev.  keep: n_objects bytes or NULL.  No table: the caller remaps its own with the map.  Needs no prior run and leaves the
 * resident labels alone. */
UMX_API int umx_labeler_relabel_dev(umx_labeler* lb, const int32_t* labels_dev, int64_t n_objects, int H, int W, const uint8_t* keep,
                                    const int32_t* pairs, int64_t n_pairs, int32_t* labels_out_dev, int32_t* map_host, int64_t* n_new);
/* Milliseconds of the last relabel call: the upload of the map, the launches, the download of the plane and the table.  Any may be
 * NULL. */
UMX_API int umx_labeler_relabel_last_ms(const umx_labeler* lb, double* upload_ms, double* kernel_ms, double* download_ms);

/*
 * Splitting touching nuclei at their necks by erosion cores (the definition is the project's
 * own).  Two nuclei are separate objects only where an unbroken line of another class lies between them; where that line has a gap
 * the labelling joins them.  With a depth D, a minimum core area C and a regrow bound L, on top of the options of a labelling run:
 *   10. objects: the kept objects (area >= A) of the plain labelling, N0 of them; M = their pixels.  Dropped objects play no part.
 *   11. erosion: E = the pixels of M whose city-block ball of radius D lies wholly in M; outside the image is not in M --
 *       scipy.ndimage.binary_erosion(M, cross, iterations=D, border_value=0).  Objects are never 4-adjacent, so every 4-connected
 *       component of E lies in one object.
 *   12. cores: the 4-connected components of E with area >= C.  An object that contains at least one is cored.
 *   13. seeds: S = the pixels of all cores and all pixels of every kept object that is not cored (it stays whole: a nucleus thinner
 *       than 2 D + 1 is never lost).  The seed objects are the 4-connected components of S, numbered 1..N in raster order of their
 *       first pixel; N >= N0.
 *   14. regrow: L synchronous levels of the growth rule above from these seeds over the domain "label 0 and pred == cls": a neck
 *       pixel goes to the core nearest through the object, a tie to the smaller label; fronts cannot leave an object, and a dropped
 *       object touches no seed.  unreached = the pixels of M still 0 after the L levels; they stay background.  (The launches stop
 *       as soon as one claimed nothing: the state is closed, so the result is that of all L levels.)
 *   15. if grow_radius > 0 the growth above over grow_classes from the labels of step 14; then the table of the final labels.
 * The result is a function of the planes and the options only; every final object contains its seed and is 4-connected; an object
 * with one core or none keeps exactly its pixels when L is large enough; a bar of width w joining two bodies is cut iff w <= 2 D.
 * Not here: merging fragments back (a ragged outline can throw small cores; C is the only guard; umx_labeler_run_hmax below places
 * the seeds by the planes' own peaks instead of by erosion).  The regrow of step 14
 * cuts a neck on the midline between its cores; umx_labeler_run_flood below cuts it along a ridge of one of the planes instead.  A split run allocates, beyond a plain run's buffers, one more int32 plane and one byte plane of H * W, kept like the others.
 */
typedef struct umx_label_split_options {
    umx_label_options base;  /* the labelling (and the rim growth of step 15) as in umx_labeler_run */
    int32_t depth;           /* D: 1 .. UMX_SPLIT_MAX_DEPTH erosion levels */
    int32_t core_min_area;   /* C: 1 .. UMX_SPLIT_MAX_CORE_AREA pixels */
    int32_t regrow;          /* L: 1 .. UMX_SPLIT_MAX_REGROW levels */
    int32_t reserved[5];     /* must be zero */
} umx_label_split_options;   /* 64 bytes */
typedef struct umx_label_split_counts {
    int64_t n_objects;       /* N: the seed objects = the objects of the result */
    int64_t n_before;        /* N0: the kept objects of the plain labelling */
    int64_t n_cored;         /* of those, the ones with at least one core */
    int64_t unreached;       /* pixels of kept objects that the L levels did not reach: background in the result */
} umx_label_split_counts;    /* 32 bytes */
/* The erosion kernel holds a halo of UMX_LABEL_GROW_HALO pixels, which bounds the depth. */
enum { UMX_SPLIT_MAX_DEPTH = 8, UMX_SPLIT_MAX_CORE_AREA = 65536, UMX_SPLIT_MAX_REGROW = 255 };
/* Host only, no device: umx_label_options_check on the base first, its message passed through unchanged; then 1 <= depth <= 8,
 * 1 <= core_min_area <= 65536, 1 <= regrow <= 255, reserved words zero.  UMX_OK, or UMX_ERR_INVALID with the reason in msg. */
UMX_API int umx_label_split_check(const umx_label_split_options* o, int K, int H, int W, char* msg, size_t cap);
/* umx_labeler_run / _run_dev with the split: the same contracts.  A refused call (UMX_ERR_INVALID) has touched nothing and leaves
 * the resident labels as they were; a successful host call with a label plane makes the split labels the resident ones, so
 * umx_labeler_measure measures them.  umx_labeler_objects, _last_ms and _last_error serve these calls too.  counts may be NULL. */
UMX_API int umx_labeler_run_split(umx_labeler* lb, const uint8_t* planes_host, int K, int H, int W, const umx_label_split_options* o,
                                  int32_t* labels_host, umx_label_split_counts* counts);
UMX_API int umx_labeler_run_split_dev(umx_labeler* lb, const uint8_t* planes_dev, int K, int H, int W, const umx_label_split_options* o,
                                      int32_t* labels_dev, umx_label_split_counts* counts);

/*
 * The level flood: the split's cut laid along a ridge of the planes (the definition is the
 * project's own).  A marker-controlled watershed by immersion, integer throughout.  On top of a split run -- whose steps 10 to 13
 * run unchanged and give the seed objects 1..N -- with a relief plane P, an invert flag and a level step q:
 *   19. relief and levels: r(p) = planes[P][p], or 255 - planes[P][p] with invert.  The levels are t_j = min(255, (j + 1) * q - 1)
 *       for j = 0 .. 256 / q - 1, in ascending order.
 *   20. flood, in place of step 14: at level t the domain is every pixel with label 0, pred == cls and r(p) <= t; synchronous
 *       steps of the growth rule (a labelled 4-neighbour of the step before, the smallest such label, every pixel deciding on the
 *       state of the step before) are repeated until one claims nothing; the next level starts from that state.  The steps have no
 *       bound: the split record's regrow must be UMX_SPLIT_MAX_REGROW in a flood call.
 *   21. rim growth, table and labels as step 15.
 * Consequences: with q = 256 there is one level, t = 255, and the result is that of umx_labeler_run_split with regrow 255 bit for
 * bit wherever that run leaves nothing unreached; N, the numbering and the seeds are the split's, every object contains its seed
 * and is 4-connected; an object with one core or none keeps exactly its pixels; two bodies joined by a neck whose relief has a
 * one-pixel-wide ridge of value v, everything else in the neck below v, are cut on the ridge wherever it stands (q small enough
 * that the ridge is alone at its level); the result is a function of the planes and the options only.  unreached is 0 for every
 * input (every kept object contains a seed and every pixel is admitted at t = 255); it is returned all the same.
 * The relief is read from the planes: a flood run allocates two words beyond a split run's buffers.
 */
typedef struct umx_label_flood_options {
    umx_label_split_options split;   /* the split run; split.regrow must be UMX_SPLIT_MAX_REGROW */
    int32_t relief_plane;            /* P: 0 .. K-1, in the model's class order */
    int32_t invert;                  /* 0: r = planes[P]; 1: r = 255 - planes[P] */
    int32_t level_step;              /* q: a power of two, 1 .. UMX_FLOOD_MAX_STEP */
    int32_t reserved[5];             /* must be zero */
} umx_label_flood_options;           /* 96 bytes */
typedef struct umx_label_flood_counts {
    int64_t n_objects, n_before, n_cored, unreached;   /* as umx_label_split_counts, in its order */
    int64_t levels_claimed;          /* levels at which at least one pixel was claimed */
    int64_t claimed;                 /* pixels claimed in all */
    int64_t launches;                /* flood launches: informative, not part of the definition */
    int64_t reserved;
} umx_label_flood_counts;            /* 64 bytes */
/* The largest level step (one level), the step of the drivers when none is given, and the steps one flood launch runs at most
 * (the halo of the growth kernel, whose geometry the flood kernel has). */
enum { UMX_FLOOD_MAX_STEP = 256, UMX_FLOOD_DEFAULT_STEP = 16, UMX_FLOOD_LAUNCH_STEPS = 8 };
/* Host only, no device: umx_label_split_check on the split record first, its message passed through unchanged; then
 * split.regrow == 255, 0 <= relief_plane < K, invert 0 or 1, level_step one of 1, 2, 4 .. 256, reserved words zero.  UMX_OK, or
 * UMX_ERR_INVALID with the reason in msg. */
UMX_API int umx_label_flood_check(const umx_label_flood_options* o, int K, int H, int W, char* msg, size_t cap);
/* umx_labeler_run_split / _run_split_dev with the flood in place of the regrow: the same contracts.  A refused call
 * (UMX_ERR_INVALID) has touched nothing and leaves the resident labels as they were; a successful host call with a label plane
 * makes the flooded labels the resident ones for umx_labeler_measure and umx_labeler_shape.  Synchronous; under UMX_DEBUG_GUARD the
 * call ends in the check of the red zones.  counts may be NULL. */
UMX_API int umx_labeler_run_flood(umx_labeler* lb, const uint8_t* planes_host, int K, int H, int W, const umx_label_flood_options* o,
                                  int32_t* labels_host, umx_label_flood_counts* counts);
UMX_API int umx_labeler_run_flood_dev(umx_labeler* lb, const uint8_t* planes_dev, int K, int H, int W, const umx_label_flood_options* o,
                                      int32_t* labels_dev, umx_label_flood_counts* counts);

/*
 * h-maxima seeds: the seed set of a flood run taken from the peaks of one of the planes instead of from erosion cores (DESIGN.md
 * section 8.1, steps 33 to 36; the definition is the project's own and integer throughout).  Erosion cores see geometry alone: two
 * nuclei joined along a front wider than 2 D are never separated, and D is bounded at 8.  With a seed plane S, an invert flag and a
 * height h on top of a flood run (whose split.depth is not used):
 *   33. seed relief: f(p) = planes[S][p] on M (the pixels of the kept objects, step 10), or 255 - planes[S][p] with seed_invert;
 *       f(p) = 0 off M and outside the image.
 *   34. h-maxima: g = the reconstruction by dilation of the marker max(f - h, 0) under the mask f, 4-connectivity: the limit of
 *       g <- min(f, max(g(p), g(its four neighbours))) started at the marker = the least function above the marker that satisfies
 *       that equation.  Objects are never 4-adjacent and f is 0 between them: nothing passes from one object to another.
 *   35. extended maxima: r = the reconstruction of max(g - 1, 0) under g; E = { p : g(p) > r(p) } = the union of the 4-connected
 *       plateaus of g with value > 0 that have no 4-neighbour of greater g.  E is a subset of M.
 *   36. steps 12 and 13 with this E in the place of the eroded set (cores: the components of E with area >= core_min_area; uncored
 *       kept objects stay whole), then steps 19 to 21 (level_step 256: the regrow by distance) and 15.
 * Consequences: (a) with core_min_area 1, n_cored = the kept objects whose largest f exceeds h; (b) h = 255 gives no core: labels,
 * table and n_objects are those of umx_labeler_run with the same base, bit for bit; (c) a relief constant and above h on M gives
 * E = M and again the plain labelling; (d) two peaks a <= b joined over a saddle s are two seeds iff a - s > h; (e) every final
 * object contains its seed and is 4-connected, N >= N0; (f) the result is a function of the planes and the options only.
 * An h-maxima run allocates what a flood run allocates and three words: the byte planes of the reconstructions live in the split's
 * third int32 plane.  Not here: seeds by a threshold on the probability, a distance-transform relief, h-maxima inside the sharded
 * schedule.
 */
typedef struct umx_label_hmax_options {
    umx_label_flood_options flood;   /* the flood run; flood.split.depth must pass the split's check and is otherwise not looked at */
    int32_t seed_plane;              /* S: 0 .. K-1, in the model's class order */
    int32_t seed_invert;             /* 0: f = planes[S]; 1: f = 255 - planes[S] */
    int32_t height;                  /* h: 1 .. UMX_HMAX_MAX_HEIGHT */
    int32_t reserved[5];             /* must be zero */
} umx_label_hmax_options;            /* 128 bytes */
typedef struct umx_label_hmax_counts {
    umx_label_flood_counts flood;    /* as umx_labeler_run_flood gives them */
    int64_t seed_pixels;             /* |E| */
    int64_t recon_launches[2];       /* launches of the reconstructions of steps 34 and 35: informative, not part of the definition */
    int64_t reserved;
} umx_label_hmax_counts;             /* 96 bytes */
/* The largest height, the steps one reconstruction launch runs at most, and the launches one reconstruction may take: a launch
 * carries a value at least UMX_LABEL_GROW_HALO pixels along any path, so a path of 16 384 pixels converges; a run that reaches the
 * bound fails (UMX_ERR_RANGE) with a message that names it. */
enum { UMX_HMAX_MAX_HEIGHT = 255, UMX_HMAX_LAUNCH_STEPS = 64, UMX_HMAX_MAX_LAUNCHES = 2048 };
/* Host only, no device: umx_label_flood_check on the flood record first, its message passed through unchanged; then
 * 0 <= seed_plane < K, seed_invert 0 or 1, 1 <= height <= 255, reserved words zero.  UMX_OK, or UMX_ERR_INVALID with the reason in
 * msg. */
UMX_API int umx_label_hmax_check(const umx_label_hmax_options* o, int K, int H, int W, char* msg, size_t cap);
/* umx_labeler_run_flood / _run_flood_dev with the h-maxima seeds in place of the erosion cores: the same contracts.  A refused call
 * (UMX_ERR_INVALID) has touched nothing and leaves the resident labels as they were; a successful host call with a label plane
 * makes the result the resident labels for umx_labeler_measure, _shape, _contacts, _hull and _relabel.  Synchronous; under
 * UMX_DEBUG_GUARD the call ends in the check of the red zones.  counts may be NULL. */
UMX_API int umx_labeler_run_hmax(umx_labeler* lb, const uint8_t* planes_host, int K, int H, int W, const umx_label_hmax_options* o,
                                 int32_t* labels_host, umx_label_hmax_counts* counts);
UMX_API int umx_labeler_run_hmax_dev(umx_labeler* lb, const uint8_t* planes_dev, int K, int H, int W, const umx_label_hmax_options* o,
                                     int32_t* labels_dev, umx_label_hmax_counts* counts);

/* Strip / tile decoders of the drivers' own TIFF reader (unmicst_amd/tiffio.py; the reference reads through tifffile /
 * imagecodecs, UnMicst1-5.py:794-797): TIFF 6.0 LZW (compression 5, the OME-TIFF / Bio-Formats default) and PackBits
 * (32773).  Host code, no device needed.  Return the decoded byte count (<= cap) or -1 on a malformed stream. */
UMX_API long long umx_tiff_lzw_decode(const uint8_t* src, size_t n, uint8_t* dst, size_t cap);
UMX_API long long umx_tiff_packbits_decode(const uint8_t* src, size_t n, uint8_t* dst, size_t cap);

/* The two halves of umx_infer_image, exposed for band sharding across GPUs (one process per GPU):
 * umx_band_tiles_dev: PI2D.getPatch + normalise + UNet for patch rows [pr0,pr1) -> probs
 *   [(pr1-pr0)*patch_cols, P,P,K] float32.  image_dev holds image rows [band_row0, band_row0+band_rows) of the
 *   full H x W image ([C_img, band_rows, W]); rows the requested patch rows need but the band lacks are an error.
 * umx_stitch_dev: PI2D.patchOutput/getValidOutput restricted to image rows [y0,y1), given the probabilities of
 *   patch rows [tpr0,tpr1) (every tile touching those rows must be inside that range) -> out [K, y1-y0, W]. */
UMX_API int umx_band_tiles_dev(umx_ctx* ctx, const double* image_dev, int C_img, int H, int W, int band_row0,
                       int band_rows, double mean, double std, int pr0, int pr1, float* probs_dev);
UMX_API int umx_stitch_dev(umx_ctx* ctx, const float* probs_dev, int tpr0, int tpr1, int H, int W, int mode, int stitch,
                   int y0, int y1, void* out_dev);

/* Per-launch-site timing with HIP events on the ctx stream (used by bench.py for the roofline object). */
typedef struct umx_prof_entry {
    char name[48];          /* layer name, e.g. "lu1.conv" */
    char kernel[64];        /* kernel instantiation as rocprofv3 names it, e.g. "conv_f16x3<9, 4, 1, false, 4, false, false, false>" */
    int64_t launches;
    double total_ms;
    double flops_per_launch_sum;  /* sum over launches of algorithmic FLOPs (no padded work counted) */
    double bytes_per_launch_sum;  /* sum over launches of compulsory HBM bytes */
    double exec_flops_sum;        /* sum over launches of FLOPs issued to the matrix cores (padding and, for
                                     UMX_PREC_F16X3, the three products per fp32 product included) */
    int64_t launches_seen;        /* every launch of the site while profiling was on; `launches` and the sums above cover the
                                     launches that were bracketed by events (all of them unless sampling) */
    int32_t xcd_order;            /* conv_f16x3 sites, last launch: workgroup order (0 plain, 1 contiguous tile run per XCD, 2 (N-block,
                                     phase) fastest inside an XCD) */
    int32_t reserved;
} umx_prof_entry;
/* on = 0: off; 1: bracket every launch with two events; N >= 2: bracket every N-th launch of each site (two events per launch
 * cost the synthetic-256 step 1.1 % -- profiles/r03/prof_event_overhead.txt -- so bench.py samples).  Resets the counters. */
UMX_API int umx_profile_enable(umx_ctx* ctx, int on);
UMX_API int umx_profile_read(umx_ctx* ctx, umx_prof_entry* entries, int max_entries, int* n_entries);
/* sizeof(umx_prof_entry) of THIS build: a binding whose mirror of the struct has another size must not call umx_profile_read
 * (the struct grew in rounds 3 and 4; unmicst_amd/umx.py checks it when it loads the library, so that two builds compared
 * through UMX_LIB cannot be decoded with the wrong stride). */
UMX_API int umx_prof_entry_size(void);

/* Host-side helpers exported for the CPU test-suite (no GPU needed): the double->float16 round-to-nearest-even
 * used by the fp16-compat stitch, and the library's view of a model (layer count, packed weight bytes, FLOPs). */
UMX_API void umx_test_double_to_half(const double* in, uint16_t* out, size_t n);
/* the same conversion by the DEVICE routine the stitch kernel uses (needs a GPU): must equal the host routine bit for bit */
UMX_API int umx_test_double_to_half_dev(const double* in, uint16_t* out, size_t n);
/* Test entries of the driver-side image kernels (--scalingFactor, --outlier, the device-side range search): each is a thin
 * wrapper around the production function on caller-given planes, so that the kernels can be held to scipy / numpy plane by
 * plane and not only through a whole network and a uint8 cast (tests/test_gpu_imagekernels.py).
 * umx_test_gauss_weights (host only): the anti-aliasing weights the resize builds for one axis, out[0] = centre tap ..
 *   out[radius]; returns the radius, or -1 (sigma <= 1e-15, radius + 1 > cap, radius beyond the resize kernel's limit). */
UMX_API int umx_test_gauss_weights(double sigma, double* out, int cap);
/* One resize [H, W] -> [h, w] of a float64 plane as the scaled path runs it (Gaussian when an axis shrinks, order-1 zoom, clip
 * to the filtered plane's range); out_f64 [h, w] and / or out_u8 [h, w] = np.uint8(255 * .), the form of the way back.
 * out_filtered [H, W] (or NULL): the plane the zoom read, i.e. the source after the Gaussian. */
UMX_API int umx_test_resize_dev(const double* src_f64, int H, int W, int h, int w, double* out_f64, uint8_t* out_u8,
                                double* out_filtered);
/* rescale_intensity(plane, (min, limit), (0, 0.983)) of n non-negative doubles: limit = max when outlier < 0, else
 * np.percentile(plane, outlier).  out_plane [n]; range2 = (min, limit). */
UMX_API int umx_test_rescale_dev(const double* plane_f64, size_t n, double outlier, double* out_plane, double* range2);
/* The device range search of the raw entry points, njobs planes per call (raw holds them back to back, bits = 8 | 16): plane j
 * of n[j] elements is copied to offset_elems[j] elements past a 256-byte-aligned device address and reduced over nslabs[j]
 * consecutive slabs (of odd length when nslabs[j] > 1), accumulating as the slab-wise upload does.  range2 [njobs][2] = (min, max). */
UMX_API int umx_test_plane_range_dev(const void* raw, int bits, const size_t* n, const size_t* offset_elems, const int* nslabs,
                                     int njobs, uint32_t* range2);
/* The drivers' uint8 cast of n float16 probabilities: out_u8 = np.uint8(255 * (np.uint8(255 * pm) * (1 / 255))) (the identity
 * grid), out_f64 = np.uint8(255 * pm) * (1 / 255) (the plane a resize back to the raw size starts from). */
UMX_API int umx_test_half_to_u8_dev(const uint16_t* half_bits, size_t n, uint8_t* out_u8, double* out_f64);
UMX_API int umx_describe(const umx_hparams* hp, int* n_launches, double* flops_per_tile, double* executed_flops_per_tile);
/* The library's wiring of a model as JSON text (host only): activation buffers (spatial size, channels), the launch list in
 * execution order -- per launch its operand groups (source buffer, channels, filter taps: concat order = group order), output
 * buffer, fused max-pool, activation, where the BatchNorm affine sits, stride-2 transposed convolution -- and the constants the
 * kernels use (BatchNorm epsilon, LeakyReLU slope).  What a reviewer compares with the graph the reference builds
 * (UnMicst1-5.py:55-237; the op graph it saves: models/<name>/model.ckpt.meta).  Writes at most cap bytes (NUL-terminated) and
 * returns in *needed the bytes the whole text takes; UMX_ERR_INVALID if cap is too small. */
UMX_API int umx_describe_graph(const umx_hparams* hp, char* json, size_t cap, size_t* needed);
/* test entry (host): one OCP MX fp6 block as the planner packs the F6 form's weights -- 32 doubles in, 24 bytes out (element i in bits
 * [6 i, 6 i + 6): e2m3, round-to-nearest-even, saturating at 7.5), returns the block's e8m0 scale byte (2^(floor(log2 max) - 2)) */
UMX_API int umx_test_mx_pack_e2m3(const double* v32, uint8_t* out24);
/* Host only (no device needed): would umx_create with UMX_PREC_F16X3 take this model?  UMX_OK, or UMX_ERR_INVALID with the first
 * refused layer and the split-precision planner's reason in umx_last_error(NULL) -- what UMX_PREC_DEFAULT falls back to the exact-fp32
 * engine on (and warns about). */
UMX_API int umx_plan_check(const umx_hparams* hp);
/* test entry (host only): the split-precision plan umx_create would make of this model (f6: UMX_PREC_F16X3_F6) under the planner's
 * switches given as arguments, not through the environment -- nt, override_list, stamps: what UMX_PLAN_NT, UMX_PLAN_OVERRIDE and
 * UMX_DEBUG_STAMPS would hold (NULL or "": not set), threads: UMX_PLAN_THREADS (0: default).  text receives one line per launch but the
 * softmax head: its UMX_DEBUG_PLAN text, the kernel instantiation, the destination buffer's layout, the N-tiles per workgroup, the weight
 * shift, a 64-bit FNV-1a digest of everything the upload would send and, for each of the nbatches batch sizes n (1 .. 4096),
 * "n:<workgroup order>/<tiles per XCD>" as a launch on n tiles would choose them.  *needed: the text's bytes with the terminator (set
 * even where cap is too small: UMX_ERR_INVALID).  A model the planner refuses: its code, the layer and reason in umx_last_error(NULL). */
UMX_API int umx_test_infer_plan(const umx_hparams* hp, int f6, int act_shift, const float* blob, size_t blob_floats, const char* nt,
                                const char* override_list, const char* stamps, int threads, const int* batches, int nbatches, char* text,
                                size_t cap, size_t* needed);
/* test entry (host only): the trainer's weight-gradient planner and kernel selection on one layer -- batch B, H x H pixels, X with Cxt
 * channels per pixel of which each slab reads Cx from channel coff[s], G with Cg channels, nslab slabs (dy, dx: tap offset, mslab: tap of
 * the master tensor); f32_route: as under UMX_TRAIN_WGRAD_F32; planes / XCs / GCs: whether the operands come with (hi, lo) planes and
 * their stored channels.  line receives the layer's UMX_DEBUG_PLAN text followed by the kernel instantiation, the launch grid, the
 * dynamic LDS bytes and how the reduce undoes the operand scales.  UMX_ERR_INVALID with the planner's reason in umx_last_error(NULL). */
UMX_API int umx_test_wgrad_plan(int B, int H, int Cxt, int Cx, int Cg, int nslab, const int* dy, const int* dx, const int* mslab,
                                const int* coff, int f32_route, int planes, int XCs, int GCs, char* line, size_t cap);
/* test entry (host only): the host pass of umx_trainer_create -- shape, parameter layout and the plan of every forward / input-gradient
 * convolution of the training step -- for batch B (<= 0: 8) and the initial parameters `blob`, on the route UMX_TRAIN_CONV_F32 (conv_f32)
 * / UMX_TRAIN_NO_KSPLIT (no_ksplit) would select.  text receives one line per convolution in build order: its UMX_DEBUG_PLAN text, then
 * its groups (channels x taps per phase @ channel offset / master dims), the fused activation, `direct`, the weight shift, the numbers of pack descriptors and weight references, the K-split scratch
 * floats and a 64-bit FNV-1a digest of everything the upload would send.  *needed: the text's bytes with the terminator (set even where
 * cap is too small: UMX_ERR_INVALID).  A shape the planner refuses: its code, the reason in umx_last_error(NULL). */
UMX_API int umx_test_train_plan(const umx_hparams* hp, int B, int conv_f32, int no_ksplit, const float* blob, size_t blob_floats,
                                char* text, size_t cap, size_t* needed);
/* test entry (host only): the stream schedule of the v2 training step as data (step_plan, unmicst_amd/csrc/umx_tstep.hip) after the
 * same host pass, with (reg != 0) or without a regulariser.  text receives one line per step in host enqueue order: "op site stream;
 * wait e..; record e..; r buf..; w buf.." -- the events its stream waits on before it and records after it, named by role and index,
 * and the buffers it reads and writes ("-": none).  The legacy graph has no schedule: UMX_ERR_INVALID. */
UMX_API int umx_test_step_plan(const umx_hparams* hp, int B, int conv_f32, int no_ksplit, int reg, const float* blob, size_t blob_floats,
                               char* text, size_t cap, size_t* needed);
/* test entries (host only): the schedule of a whole-slide call as data.  umx_test_slide_plan: what the image entries enqueue for an
 * H x W slide of C_img planes (src_bits 0: float64, 8 / 16: raw) at launch groups of max_batch tiles -- rescale, has_range (the caller
 * hands the planes' (min, max) in), sync_call (else submitted), host_range_ok (UMX_HOST_RANGE is not 0), raw_gather (the engine's tile
 * gather reads raw planes), stitch (UMX_STITCH_*), out_u8; tile_flops: algorithmic FLOPs of one tile (<= 0: from the graph of `hp`).  text
 * receives a header line (slabs, single stream or not, events, buffer cuts and sizes) and one line per step in enqueue order.
 * umx_test_band_plan: what a sharded entry enqueues for the band of `rank` in `world` -- a header line, then one line per launch group
 * (tiles, staged rows of a host band and their event) and per slab (rows, padding, event, every rank's rows) in order.  *needed: the
 * text's bytes with the terminator (set even where cap is too small: UMX_ERR_INVALID). */
UMX_API int umx_test_slide_plan(const umx_hparams* hp, int H, int W, int max_batch, int C_img, int src_bits, int rescale, int has_range,
                                int sync_call, int host_range_ok, int raw_gather, int stitch, int out_u8, double tile_flops, char* text,
                                size_t cap, size_t* needed);
UMX_API int umx_test_band_plan(const umx_hparams* hp, int H, int W, int world, int rank, int nslabs, int max_batch, int band_row0,
                               int band_rows, int stitch, int u8, int staged, int own_stream, char* text, size_t cap, size_t* needed);
UMX_API const char* umx_version(void);

#ifdef __cplusplus
}
#endif
#endif /* UMX_H */
