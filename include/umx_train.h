/*
 * umx_train.h -- C ABI of the training step of libumx.so (MI355X / gfx950 only).
 *
 * One call of umx_train_step == one `sess.run([optOp, loss], feed_dict={tfData, tfLabels, tfWeights, tfTraining: 1})`
 * of the reference's training loop (reference UnMicst1-5.py:483-484 solo, UnMicst2.py:471-472 duo): forward of the v2
 * graph with batch-statistics BN and dropout (UnMicst1-5.py:83-237), weighted cross-entropy + regularisation loss
 * (:367-373), gradients of every trainable variable, the optimiser update (:378-380) and the BN moving-average update
 * (UPDATE_OPS, :375,379).  Parameters live in the same flat blob layout umx_create takes, so a trained blob loads into
 * the inference engine unchanged.  Covered: UMX_GRAPH_V2 with nExtraConvs == 0 and 3x3 or 5x5 filters (every v2 model the
 * reference ships is 3x3), and UMX_GRAPH_LEGACY with nExtraConvs 0..2 and 3x3 or 5x5 filters -- the graph of every checkpoint the
 * reference ships with weights, trained as UnMicst.py:270-279 (train() with restoreVariables): ReLU everywhere, BN only on the
 * down blocks (on relu(conv + 1x1 shortcut), before the pool), unweighted cross-entropy, MomentumOptimizer; no dropout, no
 * regulariser (umx_train_options_legacy).
 * Conventions as in umx.h: 0 = ok, umx_trainer_last_error() gives the message, the caller owns host buffers, one
 * trainer per host thread.  There is no CPU fallback.
 */
#ifndef UMX_TRAIN_H
#define UMX_TRAIN_H

#include "umx.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct umx_trainer umx_trainer;

enum umx_optimizer { UMX_OPT_ADAM = 0, UMX_OPT_MOMENTUM = 1 };
enum umx_regulariser { UMX_REG_NONE = 0, UMX_REG_L1 = 1, UMX_REG_L2 = 2 };

/* The knobs the reference hard-codes in its scripts; umx_train_options_solo/_duo fill in those values. */
typedef struct umx_train_options {
    int32_t device_ordinal;
    int32_t batch;            /* images per step; 0 = hp.batchSize */
    int32_t optimizer;        /* enum umx_optimizer */
    int32_t decay_steps;      /* lr = lr0 * decay_rate^floor(step / decay_steps)  (tf.train.exponential_decay, staircase) */
    float lr0, decay_rate;
    float momentum;           /* MomentumOptimizer */
    float beta1, beta2, adam_eps;
    int32_t reg_kind;         /* enum umx_regulariser */
    float reg_down, reg_bottom, reg_up, reg_top;   /* coefficient on: shortcut kernels | lb kernel | lu kernels | lt kernel */
    float clip_eps;           /* > 0: log(clip(p, eps, 1-eps)) (solo, UnMicst1-5.py:369-370); 0: log(p) (duo) */
    float drop_down_step;     /* dropout rate of down layer i = drop_down_step * i          (UnMicst2.py:114) */
    float drop_bottom;        /*                 bottom layer                               (UnMicst1-5.py:139) */
    float drop_up0, drop_up_step; /*             up layer idx = drop_up0 - drop_up_step*idx (UnMicst2.py:203) */
    float bn_momentum;        /* moving-average momentum of tf.layers.batch_normalization: 0.99 */
    uint64_t seed;            /* dropout stream (counter-based hash of seed, step, layer, element) */
    int32_t reserved[8];      /* must be zero */
} umx_train_options;

UMX_API void umx_train_options_solo(umx_train_options* o);   /* UnMicst1-5.py: Adam 5e-5 x0.98/5000, l1(8e-5), bottom dropout 0.35 */
UMX_API void umx_train_options_duo(umx_train_options* o);    /* UnMicst2.py:  Adam 6e-5 x0.99/4000, l2(0.01/0.005), dropout everywhere */
UMX_API void umx_train_options_legacy(umx_train_options* o); /* UnMicst.py:   Momentum(0.9) 0.01 x0.95/1000, no regulariser, no dropout, no clip */

/* replaces UNet2D.setup + tf.global_variables_initializer / saver.restore (UnMicst1-5.py:55-237,445-449): the blob holds
 * the initial (or restored) variables incl. BN moving statistics; optimiser slots start at zero, step at 0.
 * A legacy graph with a non-zero dropout rate or reg_kind != UMX_REG_NONE is UMX_ERR_INVALID (that graph has neither), and so is
 * nClasses < 2 (the softmax of one class is 1 everywhere: its cross-entropy has no gradient). */
UMX_API int umx_trainer_create(const umx_hparams* hp, const float* weight_blob, size_t blob_floats,
                               const umx_train_options* opts, umx_trainer** out);
UMX_API void umx_trainer_destroy(umx_trainer* tr);
UMX_API const char* umx_trainer_last_error(const umx_trainer* tr);

/* ---- the initial state: tf.global_variables_initializer() of the trainer's graph, made on the device ----
 * replaces train(..., restoreVariables=False) (UnMicst2.py:434-438, UnMicst1-5.py, UnMicst.py).  Tensors are those of
 * unmicst_amd/model.py tensor_specs, in that order (t = index of the tensor there, BN tensors counted).
 *   BatchNorm     gamma 1, beta 0, moving mean 0, moving variance 1.
 *   filters       float32(z * sigma), one rounding, z a standard normal redrawn while |z| > 2 (tf.truncated_normal).
 *   sigma         legacy graph: (double)std_dev0 for every filter (UnMicst.py:83-168).  v2 graph: (double)std_dev0 for ld<i>.w1
 *                 (kernelD<i>); every other filter VarianceScaling(scale=1, mode='fan_in') of tf.compat.v1.keras, read as
 *                 sigma = sqrt(1.0 / fan_in) / UMX_INIT_TRUNC_STD with fan_in = the product of every dimension of the variable's
 *                 shape but the last (also for the transposed filters [ks, ks, Cout, Cin]); all in float64.
 *   the stream    a value depends on (seed, t, e = flat index of the element inside its tensor) only -- not on the grid, the launch
 *                 or the tensor's offset.  With mix64 the finaliser the dropout stream uses (x ^= x >> 30, *= 0xBF58476D1CE4E5B9,
 *                 x ^= x >> 27, *= 0x94D049BB133111EB, x ^= x >> 31), all arithmetic modulo 2^64:
 *                     key = mix64((seed ^ UMX_INIT_DOMAIN) + 0x9E3779B97F4A7C15 * (t + 1))
 *                 and for attempt a = 0 .. UMX_INIT_MAX_ATTEMPTS - 1, c = e * UMX_INIT_MAX_ATTEMPTS + a:
 *                     u1 = ((mix64(key ^ (2 c)) >> 11) + 1) * 2^-53   in (0, 1]
 *                     u2 =  (mix64(key ^ (2 c + 1)) >> 11) * 2^-53    in [0, 1)
 *                     z  = sqrt(-2.0 * log(u1)) * cos(UMX_INIT_TWO_PI * u2)      float64, every operation one rounding
 *                 The first attempt with |z| <= 2 is taken.  When all are refused (odds 0.0455^16, about 3e-22 per element)
 *                 z = 0: the loop on the device is bounded.
 * tests/init_ref.py restates this in numpy; device and host log / cos / sqrt may differ in the last bits, so a value may sit one
 * float32 ulp from the restatement where z * sigma falls next to a rounding boundary (tests/test_gpu_init.py). */
#define UMX_INIT_DOMAIN 0x554D58494E495431ull          /* "UMXINIT1" */
#define UMX_INIT_MAX_ATTEMPTS 16
#define UMX_INIT_TWO_PI 6.283185307179586              /* float64 nearest 2 pi, 0x401921FB54442D18 */
#define UMX_INIT_TRUNC_STD 0.87962566103423978         /* standard deviation of a standard normal truncated at +-2 */
typedef struct umx_init_options {
    uint64_t seed;            /* of the initial state only: umx_train_options.seed (the dropout stream) is not touched */
    float std_dev0;           /* the reference's stdDev0 (hp.data; 0.007 in its UNet2D.setup example, UnMicstCyto2.py:689) */
    int32_t reserved[5];      /* must be zero */
} umx_init_options;
/* The trainer's variables become the initial state (one kernel over the parameter vector); gradient vector and optimiser slots are
 * zeroed, the step counter goes to 0, a range report not yet read is dropped, and the weight scales of the split-precision
 * convolutions are re-derived from the new variables: the next step is exactly the first step of a trainer created from the blob
 * umx_trainer_read returns now.  Waits for the trainer's streams.  std_dev0 not finite or <= 0, or a non-zero reserved:
 * UMX_ERR_INVALID before anything is enqueued (the variables stay). */
UMX_API int umx_trainer_init(umx_trainer* tr, const umx_init_options* init);

/* One step on HOST buffers: data [B,P,P,nChannels], labels and weights [B,P,P,nClasses], float32 NHWC (the reference's
 * batchData / batchLabels / batchWeights, UnMicst1-5.py:455-457,483).  apply_update 0: loss and gradients only
 * (parameters, slots, moving statistics and the step counter stay).  loss3 = {total, data term, regularisation}.
 * weights == NULL (legacy trainer only): every weight 1 -- the reference's unweighted loss (UnMicst.py:276). */
UMX_API int umx_train_step(umx_trainer* tr, const float* data, const float* labels, const float* weights,
                           int apply_update, double* loss3);
/* Same on DEVICE buffers; only enqueues on the trainer's stream.  umx_trainer_loss synchronises and reads the loss. */
UMX_API int umx_train_step_dev(umx_trainer* tr, const float* data_dev, const float* labels_dev, const float* weights_dev,
                               int apply_update);
UMX_API int umx_trainer_loss(umx_trainer* tr, double* loss3);

enum umx_trainer_vector { UMX_TV_PARAMS = 0, UMX_TV_GRADS = 1, UMX_TV_SLOT_M = 2, UMX_TV_SLOT_V = 3 };
/* copy one blob-shaped vector to the host (saver.save of the variables / the gradients of the last step) */
UMX_API int umx_trainer_read(umx_trainer* tr, int which, float* out, size_t n_floats);
/* softmax output of the last step's forward pass [B,P,P,nClasses] (the reference evaluates its pixel errors on it,
 * UnMicst1-5.py:386-397) */
UMX_API int umx_trainer_probs(umx_trainer* tr, float* probs_host);
/* Diagnostics of the last step's forward pass (what sess.run would fetch by tensor name): `name` is
 *   "ld<i>.z" | "lb.z" | "lu<i>.z" | "lt.z"   the convolution output in front of that layer's BatchNorm, [B,H,W,C];
 *   "<layer>.stat"                            its batch statistics [4][C] = mean | rstd | scale = gamma rstd | shift = beta - mean scale
 *                                             (BN output = z * scale + shift: the value the LeakyReLU / max-pool decisions are taken on);
 *   "lu<i>.us"                                the up-sampled tensor behind its LeakyReLU (UnMicst1-5.py:192-195), [B,2h,2h,C];
 *   "ds<i>"                                   input of down layer i (ds0 = the batch; pooled + dropped output of layer i-1).
 * A legacy trainer's decision sites instead (every ReLU and max-pool decision is taken on one of these):
 *   "ld<i>.x<e>" | "lu<i>.x<e>"               the pre-ReLU output that extra conv e reads (e < nExtraConvs), [B,H,W,C];
 *   "ld<i>.z"                                 main chain + 1x1 shortcut, pre-ReLU;  "lu<i>.z" | "lb.z": the layer's last conv, pre-ReLU;
 *   "ld<i>.stat"                              the batch statistics of relu(z), [4][C] as above (pool decisions on relu(z)*scale + shift);
 *   "lu<i>.us"                                the up-sampled tensor behind its ReLU;  "lt.z": the logits;  "ds<i>" as above.
 * *n_floats in: capacity of `out`; out: the tensor's size (out == NULL just queries it).  Synchronises the trainer's stream.
 * The parity tests use it to take the oracle's gradient at the SAME activation / pooling decisions (tests/test_gpu_train.py). */
UMX_API int umx_trainer_read_tensor(umx_trainer* tr, const char* name, float* out, size_t* n_floats);
/* Session.run(UNet2D.nn / errors, feed_dict={tfData: batchData, tfTraining: 0}) with the trainer's current variables
 * (the validation and test passes of UNet2D.train, UnMicst1-5.py:501-502,564-565): moving statistics, no dropout.
 * data [B,P,P,nChannels] and probs [B,P,P,nClasses] are HOST buffers; synchronous. */
UMX_API int umx_trainer_eval(umx_trainer* tr, const float* data, float* probs_host);
UMX_API int64_t umx_trainer_step_count(const umx_trainer* tr);
UMX_API int umx_trainer_batch(const umx_trainer* tr);
/* algorithmic FLOPs of one step per image: forward + input gradients + weight gradients of every convolution */
UMX_API double umx_trainer_flops_per_image(const umx_trainer* tr);
/* per-phase time of the steps since the last call (ms, accumulated with HIP events when enabled) */
UMX_API int umx_trainer_profile(umx_trainer* tr, int enable, double* fwd_ms, double* bwd_ms, double* opt_ms, int* steps);
/* test entry: on != 0 makes the v2 step enqueue every step of its schedule on the main stream, in plan order, without events -- the
 * race-free statement of the same step.  The overlapped step equals it bit for bit.  (The legacy step is serial as it is.) */
UMX_API int umx_test_trainer_serial(umx_trainer* tr, int on);

/* ---- device-resident training set (unmicst_amd/csrc/umx_trainset.hip) ----
 * The reference's annotated set (I%05d_Img.tif / _Ant.tif / _wt.tif, UnMicst1-5.py:295-312, UnMicst2.py:293-309,
 * UnMicst.py:236-243) uploaded once; each step's batch is then built on the device from 32-byte descriptors. */
typedef struct umx_trainset umx_trainset;

/* The label / weight recipe: labels[k] = (code == k+1); weights[k] = intersect_weight[k] * wmap + class_weight[k] (float64, one
 * rounding; UnMicst1-5.py:276-281,306-312: W * intersectWeight + contourWeight).  weighted == 0: no weights are built and the
 * step takes the unweighted loss (legacy trainer only). */
typedef struct umx_label_weights {
    int32_t weighted;
    float class_weight[8];
    float intersect_weight[8];
    int32_t reserved[7];      /* must be zero */
} umx_label_weights;

typedef struct umx_sample_desc {  /* 32 bytes: one image of a batch */
    int32_t index, page, y0, x0;  /* sample, augmentation page, crop origin (0 <= y0, x0 <= size - imSize) */
    int32_t transform;            /* 0..7: bit 2 swaps the axes, then bit 1 flips the rows, then bit 0 flips the columns of the crop */
    float brightness, contrast;   /* data = float32((double)v * contrast + brightness), v the stored (normalised) value */
    int32_t reserved;             /* must be zero */
} umx_sample_desc;

/* n_samples samples of size x size pixels (size >= hp.imSize), each with nChannels x n_pages image planes, one annotation plane
 * and (weighted sets) one weight map, in the trainer's device memory.  Channels, classes and device come from the trainer.
 * UMX_ERR_OOM when n_samples * size^2 * (4 nChannels n_pages + 1 + 4 weighted) bytes do not fit in the free device memory;
 * UMX_ERR_INVALID for an unweighted set on a v2 trainer.  The set belongs to `tr` and must be destroyed before it. */
UMX_API int umx_trainset_create(umx_trainer* tr, int n_samples, int n_pages, int size, const umx_label_weights* lw,
                                umx_trainset** out);
/* Upload sample `index`: planes [nChannels][n_pages][size][size] float32, already normalised ((im2double(x) - mean) / std);
 * annotation [size][size] class codes (k + 1 = class k, 0 or > nClasses: unlabelled); weight_map [size][size] or NULL (= 0). */
UMX_API int umx_trainset_set(umx_trainset* ts, int index, const float* planes, const uint8_t* annotation, const float* weight_map);
UMX_API void umx_trainset_destroy(umx_trainset* ts);
/* Exactly B descriptors (host memory): assemble the batch into the trainer's own data / labels / weights buffers, then enqueue
 * the step of umx_train_step_dev on them (umx_trainer_loss reads the loss).  Every descriptor is checked first: a bad one is
 * UMX_ERR_INVALID and nothing is enqueued. */
UMX_API int umx_train_step_sampled(umx_trainer* tr, const umx_trainset* ts, const umx_sample_desc* desc, int apply_update);
/* Assemble n <= B descriptors and copy the first n images to the host: data [n,P,P,nChannels], labels and weights
 * [n,P,P,nClasses] (weights may be NULL; an unweighted set writes none).  Tests and diagnostics; synchronous. */
UMX_API int umx_trainer_assemble(umx_trainer* tr, const umx_trainset* ts, const umx_sample_desc* desc, int n, float* data,
                                 float* labels, float* weights);
/* The validation pass: assemble n <= B descriptors (rows n..B-1 zero), the eval-mode forward of umx_trainer_eval with the
 * probabilities kept on the device, then per class k: counts[k] = pixels labelled k whose argmax (first maximum) is k, counts[K + k]
 * = pixels labelled k; *loss_sum = sum over labelled pixels of -log p[label], float64 in a fixed order.  Synchronous; reports
 * the range flag as umx_trainer_eval does. */
UMX_API int umx_trainer_evaluate(umx_trainer* tr, const umx_trainset* ts, const umx_sample_desc* desc, int n, int64_t* counts,
                                 double* loss_sum);

/* ---- computed defocus and saturation ("Blur and saturation") ----
 * Per image of a batch, next to its umx_sample_desc: a blur level (index into the set's table of Gaussian kernels, 0 = none) and a
 * saturation gain >= 1 (1 = none).  Order per image and channel: page plane -> blur -> saturation -> crop + dihedral transform ->
 * brightness / contrast jitter.  Labels and weight maps are never filtered.
 *   blur        separable, edges replicated at the SAMPLE's edge (a crop in the middle of a sample sees its real neighbours):
 *               h[r][x] = float32(sum over t = -R..R, ascending, of (double)w[|t|] * (double)p[r][clamp(x + t, 0, size-1)]), then the
 *               same down the columns of h; the sum starts at 0.0, every product and every sum is one float64 rounding (no fma).
 *               Level 0 is skipped, not multiplied by w[0].
 *   saturation  only when gain != 1: r = (double)b * std + mean; r2 = min(r * gain, 1.0); s = float32((r2 - mean) / std), each
 *               operation one float64 rounding: the pixel back on the im2double scale, amplified, clipped at the sensor's ceiling. */
#define UMX_AUGMENT_MAX_LEVELS 16
#define UMX_AUGMENT_MAX_RADIUS 12
typedef struct umx_augment_table {
    float mean, std;                  /* the set's normalisation (planes hold (im2double(x) - mean) / std) */
    int32_t n_levels;                 /* 1..16; level 0 is "no blur" and must have radius 0 */
    int32_t radius[UMX_AUGMENT_MAX_LEVELS];   /* 0..12 */
    float taps[UMX_AUGMENT_MAX_LEVELS][UMX_AUGMENT_MAX_RADIUS + 1];   /* taps[l][t]: weight at distance t <= radius[l] */
    int32_t reserved[5];              /* must be zero */
} umx_augment_table;

typedef struct umx_augment_desc {     /* 8 bytes: one image of a batch, parallel to its umx_sample_desc */
    int32_t blur_level;               /* 0 .. n_levels - 1 */
    float gain;                       /* finite, >= 1 */
} umx_augment_desc;

/* Host validation of a table (no device needed): 1 <= n_levels <= 16, level 0 has radius 0, radii in 0..12, taps finite and
 * non-negative, mean finite, std finite and > 0, reserved zero.  UMX_OK, or UMX_ERR_INVALID with the broken
 * rule in msg (cap bytes, NUL-terminated; msg may be NULL). */
UMX_API int umx_augment_table_check(const umx_augment_table* table, char* msg, size_t cap);
/* Attach (or replace) the table of a set; waits for the trainer's stream first.  The table is copied. */
UMX_API int umx_trainset_set_augment(umx_trainset* ts, const umx_augment_table* table);
/* umx_train_step_sampled / umx_trainer_assemble with a parallel array of umx_augment_desc (B resp. n of them).  Checked on the host
 * like the descriptors, before anything is enqueued: UMX_ERR_INVALID for a set without a table, a level outside the table, a gain
 * that is not finite or < 1.  An image with (level 0, gain 1) is assembled exactly as the plain entries assemble it. */
UMX_API int umx_train_step_augmented(umx_trainer* tr, const umx_trainset* ts, const umx_sample_desc* desc,
                                     const umx_augment_desc* aug, int apply_update);
UMX_API int umx_trainer_assemble_augmented(umx_trainer* tr, const umx_trainset* ts, const umx_sample_desc* desc,
                                           const umx_augment_desc* aug, int n, float* data, float* labels, float* weights);

/* ---- rotation and zoom ("Rotation and zoom") ----
 * Per image of a batch, next to its umx_sample_desc (and its umx_augment_desc, when there is one): a 2 x 2 matrix, made on the host
 * in float64 and rounded to float32, M = (1 / zoom) * [[cos t, -sin t], [sin t, cos t]] (zoom > 1 magnifies).  m == {1, 0, 0, 1}
 * exactly is "no warp": such an image is assembled exactly as the entries above assemble it, blur's edge rule included.
 * Order per image and channel: page plane -> warp -> blur -> saturation -> crop orientation + dihedral transform -> jitter.  The warp
 * gives the image on the crop's own pixel grid, at every integer (y, x), also outside 0 .. P-1: the blur's halo reads those, so under
 * a warp the blur has no edge rule of its own.  With P = imSize, S = size, c = (P - 1) / 2, in float64, every product, sum, division
 * and floor one rounding (no fma):
 *   1. sy = (m[0] * (y - c) + m[1] * (x - c)) + (y0 + c);  sx = (m[2] * (y - c) + m[3] * (x - c)) + (x0 + c).
 *   2. mirror about the centres of the sample's edge pixels (d c b | a b c d | c b a), per axis: T = 2 (S - 1), q = floor(s / T),
 *      t = s - T * q, t = T - t where t > S - 1, and t = 0 where t < 0 (s / T may round up to an integer; t is then a hair below 0).
 *   3. data: i = floor(t), f = t - i, i1 = min(i + 1, S - 1) per axis; top = (1 - fx) * p[iy][ix] + fx * p[iy][ix1], bot likewise on
 *      row iy1, v = float32((1 - fy) * top + fy * bot).
 *   4. labels and the weight map: the nearest source pixel, n = min(floor(t + 0.5), S - 1) per axis, the same pixel for both; then
 *      labels[k] = (code == k+1) and weights[k] = intersect_weight[k] * wmap + class_weight[k] as in umx_label_weights.  Never
 *      interpolated, never blurred; mirrored pixels keep their (mirrored) labels. */
typedef struct umx_warp_desc {        /* 16 bytes: one image of a batch */
    float m[4];                       /* source step per output step: (sy, sx) = M (y - c, x - c) + centre of the crop */
} umx_warp_desc;

/* Host validation of n descriptors (no device needed): every entry finite and |m[i]| <= 4, determinant != 0.  UMX_OK, or
 * UMX_ERR_INVALID with the first broken one in msg (cap bytes, NUL-terminated; msg may be NULL). */
UMX_API int umx_warp_desc_check(const umx_warp_desc* warp, int n, char* msg, size_t cap);
/* umx_train_step_augmented / umx_trainer_assemble_augmented with a parallel array of umx_warp_desc (B resp. n of them).  aug == NULL:
 * no blur and gain 1 for every image, and then the set needs no table.  Everything is checked on the host before anything is
 * enqueued: UMX_ERR_INVALID for what those entries refuse, for what umx_warp_desc_check refuses, and for a set of 1-pixel samples. */
UMX_API int umx_train_step_warped(umx_trainer* tr, const umx_trainset* ts, const umx_sample_desc* desc, const umx_augment_desc* aug,
                                  const umx_warp_desc* warp, int apply_update);
UMX_API int umx_trainer_assemble_warped(umx_trainer* tr, const umx_trainset* ts, const umx_sample_desc* desc,
                                        const umx_augment_desc* aug, const umx_warp_desc* warp, int n, float* data, float* labels,
                                        float* weights);

/* ---- elastic deformation ("Elastic deformation") ----
 * Per image of a batch, next to its umx_sample_desc (and its umx_augment_desc / umx_warp_desc, when there are any): a lattice of n x n
 * displacement vectors, drawn on the host, that a uniform cubic B-spline spreads over the crop (n - 3 spline cells across it).  The
 * displacement is added to the pixel's coordinate on the crop's own grid in front of the rotation / zoom, so the image is resampled
 * once.  n == 0 is "no deformation": such an image is assembled exactly as the entries above assemble it.
 * Order per image and channel: page plane -> elastic + warp (one resampling) -> blur -> saturation -> crop orientation + dihedral
 * transform -> jitter.  For pixel (y, x) of the crop's own grid -- any integers, also outside 0 .. P-1 (the blur's halo) -- with
 * P = imSize, D = (double)d, in float64, every product, sum, division and floor one rounding (no fma):
 *   0a. per axis, t the pixel's coordinate on it: tc = min(max(t, 0), P - 1) (a pixel outside the crop takes the displacement of the
 *       nearest crop-edge pixel); scale = (double)(n - 3) / (double)(P - 1); u = tc * scale; i = min(floor(u), n - 4); f = u - i;
 *       g = 1 - f, f2 = f * f, f3 = f2 * f;  W0 = (g * g) * g;  W1 = (3 f3 - 6 f2) + 4;  W2 = ((-3 f3 + 3 f2) + 3 f) + 1;  W3 = f3
 *       (six times the B-spline's weights).
 *   0b. per component k (0: rows, 1: columns), with (Wy, iy) of y and (Wx, ix) of x:
 *       row_a = ((Wx0 D[k][iy+a][ix] + Wx1 D[k][iy+a][ix+1]) + Wx2 D[k][iy+a][ix+2]) + Wx3 D[k][iy+a][ix+3], a = 0..3;
 *       e_k = (((Wy0 row_0 + Wy1 row_1) + Wy2 row_2) + Wy3 row_3) / 36.0.   |e_k| <= max |D| (convex hull); a zero lattice gives +0.0.
 *   1'. step 1 of the warp recipe with ((y + e_0) - c) and ((x + e_1) - c) in place of (y - c) and (x - c); without a umx_warp_desc,
 *       or with the identity, the same formula with m = {1, 0, 0, 1}.
 *   2-4. as there: the mirror fold, bilinear data with one float32 rounding, label and weight from the one nearest source pixel.
 * The device draws no random number and evaluates no transcendental for this. */
#define UMX_ELASTIC_MAX_GRID 6        /* lattice points per axis: 4..6 = 1..3 spline cells across the crop */
#define UMX_ELASTIC_MAX_DISP 32.0f    /* |d| bound, pixels */
typedef struct umx_elastic_desc {     /* 304 bytes: one image of a batch, parallel to its umx_sample_desc */
    int32_t n;                        /* 0 = no elastic deformation for this image; else 4..6 */
    int32_t reserved[3];              /* must be zero */
    float d[2][6][6];                 /* d[0][a][b]: row (y) displacement of lattice point (a, b), d[1]: column (x); pixels.
                                         Entries with a >= n or b >= n must be 0 */
} umx_elastic_desc;

/* Host validation of n_desc descriptors (no device needed): n in {0, 4, 5, 6}, reserved zero, every entry finite and
 * |d| <= UMX_ELASTIC_MAX_DISP, every entry outside the n x n block zero (n == 0: all of them).  UMX_OK, or UMX_ERR_INVALID with the first
 * broken one in msg ("elastic <index> ...": cap bytes, NUL-terminated; msg may be NULL). */
UMX_API int umx_elastic_desc_check(const umx_elastic_desc* e, int n_desc, char* msg, size_t cap);
/* umx_train_step_warped / umx_trainer_assemble_warped with a parallel array of umx_elastic_desc (B resp. n of them).  aug == NULL: no
 * blur and gain 1; warp == NULL: the identity for every image; elastic == NULL is UMX_ERR_INVALID.  Everything is checked on the host
 * before anything is enqueued, in the order descriptors, augmentations (when given), warps (when given), lattices: UMX_ERR_INVALID
 * for what those entries refuse, for what umx_elastic_desc_check refuses, and for a set of 1-pixel samples. */
UMX_API int umx_train_step_elastic(umx_trainer* tr, const umx_trainset* ts, const umx_sample_desc* desc, const umx_augment_desc* aug,
                                   const umx_warp_desc* warp, const umx_elastic_desc* elastic, int apply_update);
UMX_API int umx_trainer_assemble_elastic(umx_trainer* tr, const umx_trainset* ts, const umx_sample_desc* desc,
                                         const umx_augment_desc* aug, const umx_warp_desc* warp, const umx_elastic_desc* elastic, int n,
                                         float* data, float* labels, float* weights);

/* ---- border weight maps ("Border weight maps") ----
 * For a set whose samples bring no _wt.tif: the contour-intersection map W of weights[k] = intersect_weight[k] * W + class_weight[k],
 * computed on the device from the stored annotation as the border term of Ronneberger et al. 2015 (U-Net), exp(-(d1 + d2)^2 /
 * (2 sigma^2)), d1 the distance to the nearest object and d2 to the nearest other one.  This is a reading of the published maps: the
 * reference reads them from files it never makes.  Per sample, with A its annotation [S][S], c = object_code, sg = (double)sigma:
 *   1. objects     a pixel is an object pixel iff A == c.  Components are 4-connected (UMX_BORDER_CONNECTIVITY; a one-pixel-wide
 *                  diagonal contour line separates two objects only under 4-connectivity).  label = 1 + y * S + x of the component's
 *                  first pixel in raster order; 0 off the objects.
 *   2. distances   R = ceil(4 sg) <= 32.  d1sq: the least dy^2 + dx^2 <= R^2 over object pixels (0 inside an object); d2sq: the least
 *                  over object pixels whose label differs from that of a nearest one (two components at the same least distance:
 *                  d2sq == d1sq whichever is taken first).  Integers; -1: none.  Pixels outside the sample do not exist (no mirror).
 *   3. the map     W = float32(exp(-(sqrt((double)d1sq) + sqrt((double)d2sq))^2 / (2 sg^2))) where d2sq >= 0, else 0.0f: float64,
 *                  every operation one rounding.  The cut at R drops values below exp(-8) = 3.4e-4; it is part of the definition.
 * tests/trainset_border_ref.py restates this with scipy.ndimage.label; labels, d1sq and d2sq are bit-equal to it, W within one float32
 * ulp (the device's float64 exp may differ from the host's in its last bit). */
#define UMX_BORDER_MAX_SIGMA 8.0f
#define UMX_BORDER_CONNECTIVITY 4
typedef struct umx_border_options {
    int32_t object_code;          /* the annotation code of the objects, 1..nClasses (the reference's sets: 3, nuclei) */
    float sigma;                  /* pixels, 0 < sigma <= UMX_BORDER_MAX_SIGMA */
    int32_t reserved[6];          /* must be zero */
} umx_border_options;
/* Host validation (no device needed): object_code in 1..n_classes, sigma in (0, 8] (a NaN is refused), reserved zero.  UMX_OK, or
 * UMX_ERR_INVALID with the broken rule in msg (cap bytes, NUL-terminated; msg may be NULL). */
UMX_API int umx_border_options_check(const umx_border_options* o, int n_classes, char* msg, size_t cap);
/* Replace the weight map of sample `index` (or of every sample: index == -1) by the map computed from its stored annotation.  Waits
 * for the trainer's stream before and after, like umx_trainset_set; a later umx_trainset_set of the sample overwrites the map as ever.
 * UMX_ERR_INVALID, with nothing enqueued, for an unweighted set, an index outside -1 .. n_samples-1, what umx_border_options_check
 * refuses, and samples of more than 46340 pixels a side (a label is an int32).  The first call allocates an int32 workspace of
 * n_samples * size^2 words in the set's device memory: UMX_ERR_OOM if it does not fit (umx_trainset_create does not count it). */
UMX_API int umx_trainset_border_weights(umx_trainset* ts, int index, const umx_border_options* o);
/* Diagnostics / tests, synchronous: recompute sample `index` (>= 0) with the same kernels and copy out what is asked for (any pointer
 * may be NULL), each [size][size]; the stored map is left as it was.  The first call allocates four more planes of size^2 words. */
UMX_API int umx_trainset_border_planes(umx_trainset* ts, int index, const umx_border_options* o, int32_t* labels, int32_t* d1sq,
                                       int32_t* d2sq, float* wmap);

/* ---- object score of the validation pass ("Object score") ----
 * umx_trainer_evaluate counts pixels: two nuclei merged through a three-pixel bridge cost it three pixels and are, downstream, one
 * wrong cell.  This pass counts objects instead.  The reference has only the pixel error: the definition below is this project's own,
 * as the border maps are.  Per image of a validation batch (a P x P crop), with c = object_code and min_area >= 1:
 *   1. planes      truth[y][x] = k + 1 where the assembled one-hot label of class k is 1, 0 where the pixel has no label;
 *                  pred[y][x] = 1 + argmax over the K probabilities (first maximum, as the pixel counts take it), and 0 where truth is 0:
 *                  an unlabelled pixel is outside the evaluation, as it is for the pixel error.
 *   2. objects     truth objects: the 4-connected components (UMX_BORDER_CONNECTIVITY) of truth == c; predicted objects: those of
 *                  pred == c with an area of at least min_area pixels (the smaller ones do not exist in anything below).  Objects are
 *                  taken as they appear inside the crop: one cut by the crop's edge is cut the same way on both sides.
 *                  label = 1 + y * P + x of the component's first pixel in raster order; 0 off the objects.
 *   3. overlap     for a truth object t and a kept predicted object p: I shared pixels, areas a_t and a_p.  Integer arithmetic only:
 *                    matched    pairs with 3 I > a_t + a_p            (IoU > 1/2, strictly: above one half an object has at most one
 *                                                                      partner, so no assignment step exists)
 *                    matched75  pairs with 7 I > 3 (a_t + a_p)        (IoU > 3/4)
 *                    merged     kept predicted objects p for which at least two truth objects have 2 I > a_t
 *                    split      truth objects t for which at least two kept predicted objects have 2 I > a_p
 *   4. counts      int64[UMX_OBJECT_COUNTS] = truth, predicted, matched, matched75, merged, split, 0, 0 per image; a call returns the
 *                  sum over its images.  F1 = 2 matched / (truth + predicted) is the host's to compute (NaN when both are 0).
 * tests/trainset_objects_ref.py restates this with scipy.ndimage.label; counts and labels are bit-equal to it.  On the device every
 * value is an integer sum of atomics, so no result depends on their order, and every loop is bounded. */
#define UMX_OBJECT_COUNTS 8
#define UMX_OBJECT_MAX_MIN_AREA 65536
typedef struct umx_object_options {
    int32_t object_code;          /* the class code of the objects, 1..nClasses (the reference's sets: 3, nuclei) */
    int32_t min_area;             /* predicted objects below this many pixels are dropped, 1..65536 */
    int32_t reserved[6];          /* must be zero */
} umx_object_options;
/* Host validation (no device needed): object_code in 1..n_classes, min_area in 1..65536, reserved zero.  UMX_OK, or UMX_ERR_INVALID
 * with the broken rule in msg (cap bytes, NUL-terminated; msg may be NULL). */
UMX_API int umx_object_options_check(const umx_object_options* o, int n_classes, char* msg, size_t cap);
/* Exactly umx_trainer_evaluate -- the same launches, counts and *loss_sum bit-equal to its -- and then, on the same forward pass, the
 * object pass: objects = int64[UMX_OBJECT_COUNTS], summed over the n images.  truth_codes / pred_codes: the two planes, uint8 [n][P][P]
 * each (either may be NULL; diagnostics and tests).  Every argument is checked before anything is enqueued (UMX_ERR_INVALID: what
 * umx_trainer_evaluate and umx_object_options_check refuse, a NULL objects, a tile above 4096 pixels a side).  The first call of either
 * object entry allocates the pass's workspace for B images in the set's device memory -- 26 B P^2 bytes of planes and words and 12 bytes
 * per slot of B pair tables of at least 2 P^2 slots each: UMX_ERR_OOM if it does not fit (umx_trainset_create does not count it).  It
 * is cleared on the trainer's stream at each call.  Synchronous. */
UMX_API int umx_trainer_evaluate_objects(umx_trainer* tr, umx_trainset* ts, const umx_sample_desc* desc, int n,
                                         const umx_object_options* o, int64_t* counts, double* loss_sum, int64_t* objects,
                                         uint8_t* truth_codes, uint8_t* pred_codes);
/* Diagnostics / tests, synchronous: n <= B pairs of HOST planes, uint8 [n][P][P] each, are uploaded into the same two device planes
 * (rule 1's pred = 0 where truth = 0 is applied to them on the device, by the code that applies it above) and the same launches run
 * from the labelling on.  per_image = int64[n][UMX_OBJECT_COUNTS]; truth_labels / pred_labels (either may be NULL) = int32 [n][P][P],
 * the labels of rule 2 -- of every predicted component, also of those below min_area.  No forward pass; the trainer's buffers stay. */
UMX_API int umx_trainer_object_counts(umx_trainer* tr, umx_trainset* ts, const uint8_t* truth_codes, const uint8_t* pred_codes, int n,
                                      const umx_object_options* o, int64_t* per_image, int32_t* truth_labels, int32_t* pred_labels);

/* Debug guard mode.  UMX_DEBUG_GUARD=<byte> (e.g. 0xff), read by umx_trainer_create and umx_trainset_create, gives every device
 * buffer of that trainer / set a red zone of max(64 KiB, its size rounded up to 4 KiB) on both sides.  The zones, and every buffer
 * the library does not zero or upload, are filled with that byte, so a result that depends on the byte read memory nobody wrote.
 * Every entry that enqueues work (umx_train_step, _step_dev, _step_sampled, _step_augmented, _step_warped, _step_elastic, umx_trainer_eval, _assemble,
 * _assemble_augmented, _assemble_warped, _assemble_elastic, _evaluate, umx_trainer_init, umx_trainset_set, umx_trainset_border_weights,
 * umx_trainset_border_planes, umx_trainer_evaluate_objects, umx_trainer_object_counts) then waits for the trainer's streams and checks every zone: UMX_ERR_GUARD names the buffer, the side and the
 * first and last changed byte.  Slow; for tests.  Off (unset or empty), allocations and launches are exactly the normal ones.
 *
 * The host scan of one zone (no device needed): zone_bytes bytes that should all equal `fill`, in front of (side 0) or behind
 * (side 1) a buffer of buf_bytes bytes named `label`.  UMX_OK if intact; else UMX_ERR_GUARD and, in msg (cap bytes, NUL-terminated),
 * the label, the side and the first and last changed byte as offsets from the start of the buffer (negative in front of it). */
UMX_API int umx_guard_scan(const uint8_t* zone, size_t zone_bytes, int side, size_t buf_bytes, int fill, const char* label,
                           char* msg, size_t cap);

#ifdef __cplusplus
}
#endif
#endif
