/*
 * otgan_layers.h -- layer kernels of the OT-GAN generator / critic (included from otgan.h).
 *
 * Activations are NHWC fp32, weights HWIO fp32 ([KH][KW][Cin_eff][Cout]), exactly the
 * layouts of the reference's TensorFlow graph, so parameter tensors are interchangeable.
 * Spatial sizes must be powers of two (32x32 / 64x64 images and their pyramids).
 */
#ifndef OTGAN_LAYERS_H
#define OTGAN_LAYERS_H

/* pre-activations of reference utils/nn.py:190-206 */
#define OTGAN_ACT_NONE 0
#define OTGAN_ACT_CRELU 1 /* relu(concat([x0,-x0,x1,-x1,...]))  -- doubles the channels */
#define OTGAN_ACT_CELU 2  /* elu (concat([x0,-x0,x1,-x1,...]))  -- doubles the channels */
#define OTGAN_ACT_ELU 3
#define OTGAN_ACT_RELU 4

/*
 * Geometry of one conv2d layer (reference utils/nn.py:327-338 + :234-241).
 * The (list of) input tensor(s) is ONE NHWC buffer with channel stride ldx whose first C
 * channels are the concatenated list elements; the output is written at channel offset
 * y_coff of a buffer with channel stride ldy (DenseNet blocks grow in place instead of
 * re-concatenating, reference models/densenet.py:11-16).
 * Derived: Cin_eff = C * (2 for CRELU/CELU, else 1); Hin = H << upsample;
 * OH = ceil(Hin / stride); TF 'SAME': pad_before = max((OH-1)*stride + KH - Hin, 0) / 2.
 */
typedef struct otgan_conv_desc {
  int N;        /* batch */
  int H, W;     /* stored spatial size of the input buffer */
  int C;        /* real input channels */
  int ldx;      /* channel stride of the input buffer (>= C) */
  int upsample; /* 1: 2x nearest-neighbour resize before the conv (nn.py:235-236) */
  int KH, KW;
  int stride;   /* 1 or 2 */
  int Cout;
  int ldy;      /* channel stride of the output buffer */
  int y_coff;   /* channel offset of this layer's output inside the output buffer */
  int preact;   /* OTGAN_ACT_* */
  int list_quads; /* CRELU/CELU only: 1 = every list element (or C itself for a single tensor)
                     is a multiple of 4 channels wide, i.e. aligned groups of 4 effective
                     channels map to 4 consecutive source channels with one sign -> 16-byte
                     gathers; 0 = arbitrary widths -> per-channel gathers */
  /* Optional, Winograd passes only (otgan_conv2d_filter_bytes > 0): device pointers to "amax records" of the
   * tensors the pass reads -- otgan_absmax_f32 of x (forward, wgrad) and of dy (dgrad, wgrad).  The scaled
   * two-piece operands of those passes need the largest magnitude of their source tensor; NULL = the library
   * reduces the tensor itself inside the call (one more read of it).  A caller that runs forward and wgrad on the
   * same x, or dgrad and wgrad on the same dy, computes each record once. */
  const float* x_amax;
  const float* dy_amax;
  /* forward only: 1 = y += conv(x) + bias instead of y = ...  Implemented for the 3x3 / stride-1 / 16-output growth
   * layers (dense16 kernels) and for the wide 3x3 / stride-1 layers that take the Winograd path, which is what a dense
   * block split into "wide convolutions of finished channel groups + short growth chains" needs (ops.py
   * DenseBlockFunction); any other layer with this flag set is rejected with OTGAN_ERR_INVALID. */
  int y_accumulate;
  /* Optional: device buffer of otgan_conv2d_operand_bytes(d) bytes (16-byte aligned) shared by the forward call and the
   * weight-gradient call on the SAME x.  Both passes of a Winograd layer start with the same transform of x into the
   * GEMM's operand format; with this buffer the forward call leaves that operand here instead of in its workspace
   * and the weight-gradient call reads it instead of transforming x again (the buffer must stay untouched in
   * between; x_amax is then not needed by the weight gradient).  Ignored when otgan_conv2d_operand_bytes(d) == 0;
   * when it is > 0 and a call cannot take the Winograd path (list input, misaligned operands, short workspace) the
   * call fails with OTGAN_ERR_INVALID instead of silently writing / reading nothing.  NULL = each pass transforms x. */
  void* x_operand;
  /* Optional OUTPUT amax records (round 3): the kernel that WRITES y (forward) / dx (input gradient) also leaves the
   * largest |value| it wrote in the record -- atomically max-accumulated as the float's bit pattern, so the caller must
   * have zeroed the record (all OTGAN_AMAX_RECORD_FLOATS floats) before the call; NaN / infinity propagate as in otgan_absmax_f32.  The next Winograd layer
   * takes the record as its x_amax / dy_amax and the separate reduction pass over the tensor (otgan_absmax_f32: one
   * more read of it) disappears.  otgan_conv2d_amax_fused(d, which) tells whether the pass does this inside its own
   * output kernel; otherwise a given record is filled by a separate reduction launch (same result).  Requires
   * Cout % 4 == 0 (forward) / C % 4 == 0 (input gradient), 4-aligned channel strides.  y_amax_out with y_accumulate:
   * the record receives the SUMS the call leaves in memory, so that several calls that finish different parts of a
   * buffer can share one record (the growth layers and wide convolutions of a dense block); dx_amax_out: not with
   * `accumulate` -- round 4: allowed with `accumulate` too, the record then max-accumulates the SUMS left in dx. */
  float* y_amax_out;
  float* dx_amax_out;
  /* Optional, otgan_conv2d_prepare_filters_f32 only: amax record of the NORMALISED weights the filters are made from
   * (un-folded w / wT: which = 2, 3 of the folded layers, which = 0, 1 of the strided and wide 3x3 layers), e.g. from
   * otgan_weightnorm_fwd_amax_f32.  NULL = the call reduces the weights itself (one more read of them).  Ignored for
   * filters made from FOLDED weights (a different tensor). */
  const float* w_amax;
  /* (round 4) x_amax may point to x_amax_count consecutive records (OTGAN_AMAX_RECORD_FLOATS floats apart); the bound used
   * is their maximum.  0 or 1 = one record.  Read by the growth-layer kernels (Cout = 16) and by the Winograd passes of the
   * strided 5x5 and the wide 3x3 stride-1 layers (as is dy_amax_count below); every other pass reads the first record only. */
  int x_amax_count;
  /* (round 4) CRELU / CELU list inputs: nonzero = every list element is exactly this many channels wide and lies at channel
   * i * list_width of x, i.e. the channel map is the per-element interleave [x_0, -x_0, x_1, -x_1, ...] of equal slices.
   * With list_width = 16, CRELU, y_accumulate, no bias, an x_amax record and `filters` prepared by
   * otgan_dense16_prepare_filters_f32, a growth layer (3x3, stride 1, Cout = 16) runs on the two-scaled-fp16-piece kernel
   * (otgan_dense16_h2_ok tells).  0 = unknown (the channel map decides). */
  int list_width;
  /* (round 4) forward only: the layer is followed by a gated linear unit over the channel halves (reference
   * models/dcgan.py:35-36: a, b = split(y, 2, axis = 3); a * sigmoid(b)).  Non-NULL glu_out: the kernel that writes y
   * also writes the gated product to glu_out[N, OH, OW, Cout / 2] (contiguous, 16-byte aligned) -- y itself is still
   * written, the backward pass of the unit needs it -- and, if glu_amax_out is non-NULL, max-accumulates the largest
   * |gated value| into that (zeroed) amax record.  Only where otgan_conv2d_glu_fused(d) returns 1 (the Winograd path of
   * the 5x5 upsampling layers, Cout % 8 == 0, y_coff == 0, ldy == Cout); any other layer with glu_out set is rejected
   * with OTGAN_ERR_INVALID.  Same arithmetic as otgan_glu_fwd_amax_f32 on y: bit-identical. */
  float* glu_out;
  float* glu_amax_out;
  /* (round 4) dy_amax points to this many consecutive records (see x_amax_count); 0 or 1 = one record. */
  int dy_amax_count;
} otgan_conv_desc;

/*
 * Channel maps (device int32 arrays, may be NULL for a single-tensor input):
 *   cmap[d], d in [0, Cin_eff): source channel (low 31 bits) and sign (bit 31 set = negate)
 *            of effective channel d -- encodes the reference's per-list-element interleave
 *            [x0,-x0,x1,-x1,...] (nn.py:198,200).  NULL = [x, -x] / identity.
 *   inv[c], inv[C + c]: effective index of (+x_c) and (-x_c); used by dgrad.  NULL = c, C+c.
 */

/* which: 0 fwd, 1 dgrad, 2 wgrad */
size_t otgan_conv2d_workspace_bytes(const otgan_conv_desc* d, int which);
/* 1: the forward pass of this layer can write the gated product of otgan_conv_desc::glu_out itself */
int otgan_conv2d_glu_fused(const otgan_conv_desc* d);
/* size of otgan_conv_desc::x_operand for this layer; 0 = forward and weight gradient do not share an operand */
size_t otgan_conv2d_operand_bytes(const otgan_conv_desc* d);

/*
 * amax record of x[rows][C] (row stride ld floats, C and ld multiples of 4, 16-byte aligned): the largest |x| (NaN if
 * any element is NaN).  record: OTGAN_AMAX_RECORD_FLOATS floats of device memory, written asynchronously on `stream`;
 * pass it as otgan_conv_desc::x_amax / dy_amax.  Deterministic.  Format: 16 sub-slots at a stride of 32 floats, each
 * the bit pattern of a non-negative float; the record's value is their maximum (this call writes it to sub-slot 0 and
 * zeroes the others; the kernels behind y_amax_out / dx_amax_out max-accumulate into all 16, one cache line each, so
 * that their atomics do not queue up in one L2 channel).
 */
#define OTGAN_AMAX_RECORD_FLOATS 512
int otgan_absmax_f32(const float* x, long rows, int C, long ld, float* record, void* stream);
/* which: 0 forward (y_amax_out), 1 input gradient (dx_amax_out): 1 = the pass fills the record in its own output
 * kernel (no extra launch, no extra read), 0 = it would take a separate reduction. */
int otgan_conv2d_amax_fused(const otgan_conv_desc* d, int which);

/*
 * Winograd F(4x4,3x3) paths (fwd, dgrad and wgrad; scratch for the transformed operands is
 * reported by otgan_conv2d_workspace_bytes; nothing else changes for the caller):
 *   - folded 5x5 upsampling layers without pre-activation (the DCGAN generator,
 *     models/dcgan.py:33-46): each output-parity class is a 3x3 convolution on the small image;
 *   - 5x5 stride-2 layers with a single-tensor input (the DCGAN critic, models/dcgan.py:12-14):
 *     four 3x3 sub-convolutions of the input-parity sub-images, classes folded into the
 *     contraction index, structurally-zero blocks skipped (49 instead of 100 products per tile).
 *   - 3x3 stride-1 layers with >= 128 outputs and a single-tensor input (the wide convolutions a dense block is cut
 *     into, ops.py DenseBlockFunction) and 3x3 layers on a 2x upsampled input with CReLU (the DenseNet generator's
 *     transitions, models/densenet.py:67-73): the same passes with one class on the (upsampled) grid.
 * The batched GEMMs of these paths run on the fp16 matrix pipe with operands stored as two fp16 pieces of the
 * power-of-two-scaled value (hi + lo = 22 significand bits, one scale per Winograd frequency derived from the
 * largest magnitude of the tensor the operand is a transform of): three MFMAs per product, fp32 accumulation,
 * exact rescale on the way out -- measured errors at or below those of the fp32 MFMA chain of the direct path.
 * OTGAN_WINO_PIECES=3 selects the other build of the same source: three bf16 pieces (24 significand bits), six
 * MFMAs per product, no scales (read per call; a prepared filter buffer belongs to the mode it was made in).
 * Environment switches (debugging / A-B measurements): OTGAN_DISABLE_WINOGRAD=1,
 * OTGAN_WINO_FP32=1 (Winograd GEMMs on the fp32 engine), OTGAN_WINO_WGRAD_X3=0 (weight-gradient GEMMs on
 * the fp32 engine), OTGAN_WINO_WGRAD_TL=0 (weight-gradient operands from the transposing producers instead
 * of the forward-layout ones), OTGAN_DISABLE_DENSE16=1, OTGAN_DENSE16_V1=1; tuning knobs kept for measurements:
 * OTGAN_X3_SPLIT_TARGET (workgroups a K-split weight-gradient GEMM aims for, default 256), OTGAN_OUTER_CHUNKS
 * (pixel chunks of the few-channel weight gradient, default 512), OTGAN_X3_STREAM (0 / 1 / 2: the persistent
 * stream-K GEMM never / where it pays / always; read per launch), OTGAN_X3_STREAM_HALF_ROUNDS (its selection
 * threshold in half tiles per compute unit, default 3), OTGAN_X3_FMAP=0 (tile-residue instead of frequency-major
 * GEMM grid), OTGAN_AMAX_BLOCKS (workgroups of the largest-magnitude reduction, default 256);
 * OTGAN_DISABLE_WINO_PLAIN3=1 (wide 3x3 stride-1 layers back on the implicit GEMM), OTGAN_PLAIN3_MIN_CEFF / _MIN_COUT
 * (their eligibility thresholds, 64 / 128), OTGAN_DISABLE_WINO_UP3=1, OTGAN_DISABLE_WINO_UP3_WGRAD=1,
 * OTGAN_DISABLE_WINO_UP3_DGRAD=1 (3x3 upsampling layers: all passes / weight gradient / input gradient back on the
 * folded implicit GEMM), OTGAN_DISABLE_X_OPERAND=1 (otgan_conv2d_operand_bytes reports 0: no operand sharing),
 * OTGAN_IGEMM_X3=0 (implicit-GEMM forward / input gradient back on the fp32 MFMA loop instead of three bf16 pieces).
 */

/*
 * Upsample folding.  conv(k x k) applied to a 2x nearest-neighbour upsampled image equals four
 * output-parity-class convolutions on the SMALL image whose taps are sums of the original
 * ones (k = 5: 3x3 per class instead of 5x5; k = 3: 2x2 instead of 3x3) -- identical
 * mathematics with 25/9 (9/4) fewer multiply-adds in fwd, dgrad and wgrad.
 * A layer is folded iff otgan_conv2d_folded_weight_elems(d) > 0 (a pure function of the
 * descriptor: upsample == 1, stride == 1, Cin_eff % 16 == 0, 4-aligned channel strides).
 * For a folded layer the caller runs otgan_conv2d_fold_weights_f32 once per weight update and
 * passes `weffT` as the `wT` argument of otgan_conv2d_fwd_f32 and `weff` as the `w` argument
 * of otgan_conv2d_dgrad_f32; otgan_conv2d_wgrad_f32 still returns the un-folded HWIO gradient.
 */
size_t otgan_conv2d_folded_weight_elems(const otgan_conv_desc* d);
int otgan_conv2d_fold_weights_f32(const otgan_conv_desc* d, const float* w, float* weff,
                                  float* weffT, void* stream);

/*
 * The three passes below: what a pass does when a call does not meet the requirements of the layer's fast route (pinned by
 * tests/test_conv_routes_gpu.py; pointers 16-byte aligned, pitches multiples of 4, a single-tensor input, a workspace of the
 * size queried):
 *   - 5x5 stride-2 and wide 3x3 stride-1 layers (Winograd): every pass falls back to the implicit GEMM, same result;
 *     so do the 3x3 upsampling layers' weight gradient and, without `filters`, their forward / input gradient.
 *   - folded 5x5 upsampling layers (Winograd) never fall back: misaligned operands / lddx % 4 != 0 are OTGAN_ERR_INVALID,
 *     a NULL or short workspace is OTGAN_ERR_WORKSPACE.  3x3 upsampling layers called WITH `filters`: OTGAN_ERR_INVALID
 *     for either (forward and input gradient).  Other folded layers need 16-byte aligned x and wT in the forward pass.
 *   - input gradient through an un-folded 2x upsample, weight gradients that split their pixels, of folded layers and of
 *     few-channel layers (Cout <= 4, or Cin_eff <= 4 without pre-activation): OTGAN_ERR_WORKSPACE on a NULL or short
 *     workspace.  A weight gradient on float4 gathers (Cin_eff >= 32, everything a multiple of 4) needs 16-byte aligned x
 *     and dy: OTGAN_ERR_INVALID otherwise.
 *   - everything else (misaligned y / bias / dx / dw, odd pitches and channel counts, a NULL workspace elsewhere) only
 *     selects slower kernels, which read and write nothing outside the rows the descriptor describes.  A refused call
 *     writes nothing.
 */
/* y = conv2d(preact(upsample(x)), W) + bias.   wT: [Cout][KH*KW*Cin_eff] (transposed copy
 * of the HWIO weight, produced by otgan_weightnorm_fwd_f32).  nn.py:241,337. */
int otgan_conv2d_fwd_f32(const otgan_conv_desc* d, const float* x, const int32_t* cmap,
                         const float* wT, const float* bias, float* y, void* workspace,
                         size_t workspace_bytes, void* stream);

/* dx (+)= d(loss)/d(x) given dy; w is the HWIO weight.  x (the layer input) is needed for
 * the activation derivative.  dx: [N,H,W,lddx] (first C channels written).
 * accumulate != 0 adds into dx (DenseNet gradient buffers). */
int otgan_conv2d_dgrad_f32(const otgan_conv_desc* d, const float* dy, const float* w,
                           const float* x, const int32_t* inv, float* dx, int lddx,
                           int accumulate, void* workspace, size_t workspace_bytes, void* stream);

/*
 * Winograd-domain filters made once per weight update.  The layers that run as Winograd GEMMs derive
 * their filter operand from the weights inside every forward / dgrad call; a caller that knows the
 * weights are unchanged (the critic during the generator steps: five steps out of six) can derive it
 * once into its own buffer and pass it to the _pf variants.
 *   otgan_conv2d_filter_bytes(d, which)   which = 0 forward, 1 dgrad; 0: the layer / pass has none
 *   otgan_conv2d_prepare_filters_f32      `w` = what the pass itself takes (wT for forward, w for dgrad;
 *                                         folded layers: weffT / weff).  Folded layers also accept
 *                                         which = 2 / 3: forward / dgrad filters from the UN-folded wT / w
 *                                         (bit-identical; the fold is then not needed by these two passes:
 *                                         with `filters` given they do not read their weight argument).
 *                                         3x3 layers on an upsampled CReLU input have ONLY these two (their
 *                                         forward / dgrad run as Winograd GEMMs exactly when `filters` is given;
 *                                         a forward or dgrad call with `filters` must then satisfy that path's
 *                                         alignment / workspace requirements -- it is rejected otherwise, never rerouted)
 *   otgan_conv2d_fwd_pf_f32 / otgan_conv2d_dgrad_pf_f32: as the plain calls; `filters` may be NULL
 *                                         (then identical to them) and is ignored by the non-Winograd paths.
 * The buffer's content is tied to the descriptor and to the OTGAN_WINO_* switches of the process.
 */
size_t otgan_conv2d_filter_bytes(const otgan_conv_desc* d, int which);
/* Growth layers of a split dense block (ops.py DenseBlockFunction): the chain weights wT [16][9 * 32 * nslices] (CReLU over
 * `nslices` list elements of 16 channels) pre-split into two scaled fp16 pieces in MFMA fragment order, up to
 * OTGAN_DENSE16_MAX_BATCH layers per launch; pass the buffer as `filters` of otgan_conv2d_fwd_pf_f32.
 * otgan_dense16_h2_ok(d): 1 if a forward call with this descriptor (plus filters and x_amax) takes that kernel. */
#define OTGAN_DENSE16_MAX_BATCH 16
size_t otgan_dense16_filter_bytes(int nslices);
int otgan_dense16_prepare_filters_f32(const float* const* wT, const int* nslices, void* const* filters, int count,
                                      void* stream);
int otgan_dense16_h2_ok(const otgan_conv_desc* d);
/*
 * Input gradient of those chains BY SLICE (round 4): the gradient of slice c of a group gathers from the `npairs` later
 * layers of the group in one launch,  dG_c += [x_c > 0] G+ - [x_c < 0] G-  (CReLU; reference utils/nn.py:198-200 backward),
 * instead of every layer adding into every earlier slice.  g / dx: the gradient buffer [N, H, W, ldg] at the first channel of
 * slice c + 1 / of slice c; x: the forward buffer at slice c (row stride ldx).  Slices must be processed last to first
 * (a source slice must be final).  filters: otgan_dense16_bwd_filter_bytes(npairs) bytes prepared by
 * otgan_dense16_prepare_bwd_filters_f32 -- one otgan_dense16_bwd_pair per (output slice, source layer): `w` the source
 * layer's chain weights HWIO [9][32 * nslices_src][16], `fwd_filters` that layer's forward buffer (scale exponent),
 * `slice_index` the position of slice c in that chain, `pair_index` the pair's position in `filters`;
 * all_fwd_filters: the forward buffers of every chain layer of the block (one scale for the block).
 * rec0 / rec1: two ranges of consecutive amax records whose maximum bounds the source slices (rec1 nullable);
 * amax_out (nullable, zeroed or shared): max-accumulates the sums written.  Geometry as otgan_dense16_h2_ok.
 */
/*
 * Whole chains in one call (the launches of a group's layers issued back to back from C: at 8 x 8 a chain kernel takes 9 us,
 * less than one Python-level call).  A group = `nslices` consecutive 16-channel slices of the block buffer starting at
 * `buf_group` (row stride ld floats); records = (nslices + 1) consecutive amax records [W, c_0, c_1, ...] as laid out by
 * ops.py DenseBlockFunction (W: the wide convolutions' sums; c_j: left by the kernel that finishes slice j).
 *   otgan_dense16_chain_fwd_f32: layers j = 1 .. nslices - 1 in order, layer j adds its chain over slices [0, j) onto slice
 *     j (filters[j - 1]: its prepared weights), reads records [0, 1 + j), writes record 1 + j.
 *   otgan_dense16_chain_bwd_f32: slices c = nslices - 2 .. 0, otgan_dense16_bwd_slice_f32 each (filters[c]; sources bounded
 *     by rec0 (one record) and slice_records[c + 1 ..]; slice_records[c] receives the sums left).
 */
int otgan_dense16_chain_fwd_f32(int N, int H, int W, int nslices, float* buf_group, int ld, const void* const* filters,
                                float* records, void* stream);
int otgan_dense16_chain_bwd_f32(int N, int H, int W, int nslices, float* g_group, int ldg, const float* x_group, int ldx,
                                const void* const* filters, const float* rec0, float* slice_records, void* stream);
typedef struct otgan_dense16_bwd_pair {
  const float* w;
  const void* fwd_filters;
  void* filters;
  int nslices_src, slice_index, pair_index;
} otgan_dense16_bwd_pair;
size_t otgan_dense16_bwd_filter_bytes(int npairs);
int otgan_dense16_prepare_bwd_filters_f32(const otgan_dense16_bwd_pair* pairs, int npairs, const void* const* all_fwd_filters,
                                          int nall, void* stream);
int otgan_dense16_bwd_slice_f32(int N, int H, int W, int npairs, const float* g, int ldg, const void* filters, const float* x,
                                int ldx, float* dx, const float* rec0, int nrec0, const float* rec1, int nrec1,
                                float* amax_out, void* stream);
int otgan_conv2d_prepare_filters_f32(const otgan_conv_desc* d, int which, const float* w, void* filters,
                                     size_t filter_bytes, void* stream);
/* The same filters from the RAW weight-norm direction V[KH*KW][Cin_eff][Cout] (HWIO) and scale[Cout] = g * inv_norm
 * (otgan_weightnorm_scale_amax_f32), bit-identical to the ones otgan_conv2d_prepare_filters_f32 makes from the normalised
 * w / wT -- which a caller on this route never writes.  Same `which` values, same refusals by the same codes; it needs
 * otgan_conv_desc::w_amax, and which = 0 / 1 of a FOLDED layer (filters from the folded weights) is OTGAN_ERR_UNSUPPORTED. */
int otgan_conv2d_prepare_filters_raw_f32(const otgan_conv_desc* d, int which, const float* V, const float* scale,
                                         void* filters, size_t filter_bytes, void* stream);
int otgan_conv2d_fwd_pf_f32(const otgan_conv_desc* d, const float* x, const int32_t* cmap,
                            const float* wT, const void* filters, const float* bias, float* y,
                            void* workspace, size_t workspace_bytes, void* stream);
int otgan_conv2d_dgrad_pf_f32(const otgan_conv_desc* d, const float* dy, const float* w, const void* filters,
                              const float* x, const int32_t* inv, float* dx, int lddx,
                              int accumulate, void* workspace, size_t workspace_bytes, void* stream);

/* dw[KH][KW][Cin_eff][Cout] = sum over pixels of preact(x)^T . dy  (overwrites dw). */
int otgan_conv2d_wgrad_f32(const otgan_conv_desc* d, const float* x, const int32_t* cmap,
                           const float* dy, float* dw, void* workspace, size_t workspace_bytes,
                           void* stream);

/* ---- weight normalisation (nn.py:176-181): w = g * V * rsqrt(max(sum_col V^2, 1e-12)) ------------
 * V, w: [K][Cout] (K = KH*KW*Cin_eff), wT: [Cout][K] (nullable), inv_norm: [Cout].        */
int otgan_weightnorm_fwd_f32(const float* V, const float* g, int K, int Cout, float* w,
                             float* wT, float* inv_norm, void* stream);
/* the same, also max-accumulating |w| into an amax record (zeroed by the caller; NULL = none): pass it as
 * otgan_conv_desc::w_amax to otgan_conv2d_prepare_filters_f32 */
int otgan_weightnorm_fwd_amax_f32(const float* V, const float* g, int K, int Cout, float* w, float* wT,
                                  float* inv_norm, float* w_amax, void* stream);
/* What otgan_weightnorm_fwd_amax_f32 leaves beside w, without writing w: inv_norm (bit-identical: same reduction), scale[c] =
 * g[c] * inv_norm[c] (the factor w = V * scale is rounded with) and the amax record of that never-materialised w, from ONE
 * pass over V (column sums of squares and column maxima of |V|) and a finish launch.  w_amax: zeroed by the caller;
 * scratch: otgan_weightnorm_scale_scratch_floats(K, Cout) floats, 16-byte aligned. */
size_t otgan_weightnorm_scale_scratch_floats(int K, int Cout);
int otgan_weightnorm_scale_amax_f32(const float* V, const float* g, int K, int Cout, float* inv_norm, float* scale,
                                    float* w_amax, float* scratch, size_t scratch_floats, void* stream);
/* dV, dg from dw (scratch: Cout floats). */
int otgan_weightnorm_bwd_f32(const float* V, const float* g, const float* inv_norm,
                             const float* dw, int K, int Cout, float* dV, float* dg,
                             float* scratch, void* stream);

/*
 * The same two passes for MANY layers with 16 outputs each (the growth layers of a dense block,
 * models/densenet.py:11-16) in one launch per OTGAN_WN_MAX_LAYERS layers: `layers` is a HOST array, the pointers in it
 * are device pointers (16-byte aligned).  Deterministic.
 *   forward: w[K][16], wT[16][K] (nullable), inv[16] from V[K][16], g[16].
 *   backward: dV[taps*Ceff][16], dg[16] from the weight gradient given as up to three PARTS per layer, each holding
 *     nrows consecutive effective-channel rows of every tap: row (tap, e) of part i is the 16 floats at
 *     p + ((tap * nrows + perm[e]) * rstride)   (perm: device int32 array or NULL = identity; unused parts: nrows 0)
 *     -- the layout in which a dense block computed as wide convolutions + growth chains (ops.py DenseBlockFunction)
 *     leaves its weight gradients: a column slice of each wide convolution's dw, then the layer's own chain.
 */
#define OTGAN_WN_MAX_LAYERS 16
typedef struct otgan_wn_fwd_layer {
  const float* V;
  const float* g;
  float* w;
  float* wT;
  float* inv;
  int K;
} otgan_wn_fwd_layer;
typedef struct otgan_wn_part {
  const float* p;
  const int32_t* perm;
  int nrows;
  int rstride;
} otgan_wn_part;
typedef struct otgan_wn_bwd_layer {
  const float* V;
  const float* g;
  const float* inv;
  float* dV;
  float* dg;
  int Ceff, taps;
  otgan_wn_part part[3];
} otgan_wn_bwd_layer;
int otgan_weightnorm_fwd_batched16_f32(const otgan_wn_fwd_layer* layers, int n_layers, void* stream);
int otgan_weightnorm_bwd_batched16_f32(const otgan_wn_bwd_layer* layers, int n_layers, void* stream);

/* out[c] = sum_r a[r*lda + c]   (bias gradients; rows = pixels).  scratch: 256*cols floats */
int otgan_colsum_f32(const float* a, long rows, int cols, long lda, float* out, float* scratch,
                     void* stream);

/* ---- pointwise blocks ------------------------------------------------------------------ */
/* GLU (models/dcgan.py:35-36): y[r, c] = x[r, c] * sigmoid(x[r, C + c]), x: [rows, 2C].    */
int otgan_glu_fwd_f32(const float* x, long rows, int C, float* y, void* stream);
int otgan_glu_bwd_f32(const float* x, const float* dy, long rows, int C, float* dx, void* stream);
/* the same, also max-accumulating |y| / |dx| into an amax record (otgan_conv_desc::y_amax_out; NULL = none;
 * needs C % 4 == 0 and 16-byte aligned tensors) */
int otgan_glu_fwd_amax_f32(const float* x, long rows, int C, float* y, float* y_amax, void* stream);
int otgan_glu_bwd_amax_f32(const float* x, const float* dy, long rows, int C, float* dx, float* dx_amax, void* stream);
/* The same, also writing colsum[2 C] = the column sums of dx (the bias gradient of the convolution in front of the GLU,
 * models/dcgan.py:39-47: conv -> GLU) without another pass over dx.  scratch: 256 * 2 C floats.  C % 4 == 0, 16-byte
 * aligned tensors; dx_amax nullable. */
int otgan_glu_bwd_colsum_f32(const float* x, const float* dy, long rows, int C, float* dx, float* dx_amax, float* colsum,
                             float* scratch, void* stream);
/* tanh output (models/dcgan.py:50) */
int otgan_tanh_fwd_f32(const float* x, long n, float* y, void* stream);
int otgan_tanh_bwd_f32(const float* y, const float* dy, long n, float* dx, void* stream);
/* Feature head (models/dcgan.py:16-19): f = concat([relu(x), relu(-x)], channel), flatten
 * (h, w, c), L2-normalise rows (no epsilon).  x: [N, HW, C] -> f: [N, HW*2C].
 * norm: [N] saved row norms for the backward pass. */
int otgan_feature_head_fwd_f32(const float* x, int N, int HW, int C, float* f, float* norm,
                               void* stream);
int otgan_feature_head_bwd_f32(const float* x, const float* f, const float* norm,
                               const float* df, int N, int HW, int C, float* dx, void* stream);
/* the same, also max-accumulating |dx| into an amax record (NULL = none) */
int otgan_feature_head_bwd_amax_f32(const float* x, const float* f, const float* norm, const float* df, int N, int HW,
                                    int C, float* dx, float* dx_amax, void* stream);

/* ---- optimiser / EMA (utils/nn.py:50-73, train.py:63-64) --------------------------------
 * Adam with the reference's epsilon placement:  p -= lr * vhat / sqrt(mghat + 1e-8),
 * vhat = v/(1-mom1^t), mghat = mg/(1-mom2^t); mom1 == 0 skips the first moment.          */
/* Hyper-parameters travel as doubles: the reference forms (1 - mom) and (1 - mom^t) in
 * Python doubles before they become fp32 graph constants.                                  */
int otgan_adam_step_f32(float* p, const float* grad, float* v, float* mg, long n, double lr,
                        double mom1, double mom2, double t, void* stream);
/* The same step over a FLAT parameter buffer p whose gradient comes as one device tensor per variable (what the
 * backward pass returns): variable i owns p[offsets[i] .. offsets[i+1]) and reads grads[i][0 ..]; `grads` and `offsets`
 * (nseg + 1 entries, ascending) are HOST arrays, nseg <= OTGAN_ADAM_MAX_SEGMENTS.  No concatenation of the gradients
 * (151 MB per DCGAN generator step).  ema_shadow (nullable, same layout as p): shadow = ema_decay * shadow +
 * (1 - ema_decay) * p_new in the same pass (train.py:63-64,223). */
#define OTGAN_ADAM_MAX_SEGMENTS 32
int otgan_adam_step_gather_f32(float* p, const float* const* grads, const long* offsets, int nseg, float* v, float* mg,
                               double lr, double mom1, double mom2, double t, float* ema_shadow, double ema_decay,
                               void* stream);
/* The bias corrections {1 - mom1^t, 1 - mom2^t} of that step as the two entries above evaluate them (fp32, nn.py:62,67), on
 * the HOST (no launch), and the gathered step reading them from DEVICE memory (`coef_dev` [2]; null = from `t` as above):
 * a step captured in a hipGraph (trainer.py: one graph per step kind, replayed) keeps its launch arguments, so what changes
 * from step to step must come from memory -- the trainer writes the next step's pair into `coef_dev` before each replay and
 * the replayed step is bit-identical to the eager one (reference train.py:142-143: one `t` per optimiser). */
void otgan_adam_coefficients(double mom1, double mom2, double t, float* out2);
int otgan_adam_step_coef_f32(float* p, const float* grad, float* v, float* mg, long n, double lr,
                             double mom1, double mom2, double t, const float* coef_dev, void* stream);
int otgan_adam_step_gather_coef_f32(float* p, const float* const* grads, const long* offsets, int nseg, float* v, float* mg,
                                    double lr, double mom1, double mom2, double t, const float* coef_dev, float* ema_shadow,
                                    double ema_decay, void* stream);
/* Up to OTGAN_COPY2D_MAX_SEGMENTS strided 2-D copies in ONE launch: dst[s][r * dst_ld[s] + c] = src[s][r * src_ld[s] + c]
 * for r < rows[s], c < cols[s].  All arrays are HOST arrays of nseg entries.  (The growth layers of a DenseNet block read
 * sub-blocks of their normalised weights -- rows of every filter tap, models/densenet.py:11-16 through
 * ops.py DenseBlockFunction -- as contiguous tensors: 28 slices per block and weight version, one launch instead of
 * 28 framework copies.) */
#define OTGAN_COPY2D_MAX_SEGMENTS 64
int otgan_copy2d_batched_f32(const float* const* src, float* const* dst, const int* rows, const int* cols,
                             const long* src_ld, const long* dst_ld, int nseg, void* stream);
/* Up to OTGAN_GATHER3D_MAX_SEGMENTS strided 3-D copies with a gathered middle index in ONE launch:
 *   dst[s][i0 * dst_s0[s] + i1 * dst_s1[s] + i2] = src[s][i0 * src_s0[s] + (base1 + map1[i1]) * src_s1[s] + i2]
 * for i0 < n0[s], i1 < n1, i2 < n2 (map1: n1 device ints, or NULL = identity); the per-segment arrays are HOST arrays of nseg
 * entries, strides in elements.  (The wide convolutions of a split DenseNet block -- reference models/densenet.py:11-16 through
 * ops.py _split_block_plan -- read the rows of one channel group out of the weights of all later growth layers, side by side
 * and re-ordered from the reference's per-list-element CReLU order [x0, -x0, x1, -x1, ...] (utils/nn.py:198-200) to the
 * single-tensor order: one launch per operand instead of a cat, an index_select and their copies per layer.)  amax_out
 * (nullable): a zeroed amax record (OTGAN_AMAX_RECORD_FLOATS floats) that receives the largest magnitude written -- the
 * record `otgan_conv_desc::w_amax` wants for the gathered weights, without a reduction pass over them. */
#define OTGAN_GATHER3D_MAX_SEGMENTS 32
int otgan_gather3d_batched_f32(const float* const* src, float* const* dst, const int* n0, int n1, int n2,
                               const long* src_s0, const long* src_s1, const long* dst_s0, const long* dst_s1,
                               int base1, const int* map1_dev, float* amax_out, int nseg, void* stream);
int otgan_adamax_step_f32(float* p, const float* grad, float* v, float* mg, long n, double lr,
                          double mom1, double mom2, void* stream);
int otgan_nesterov_step_f32(float* p, const float* grad, float* v, long n, double lr, double mom1,
                            void* stream);
/* shadow = decay*shadow + (1-decay)*p */
int otgan_ema_update_f32(float* shadow, const float* p, long n, double decay, void* stream);

/*
 * Inception-v3 inference (the 2015 graph of the reference's evaluation, utils/inception.py; lowered by
 * utils/inception_net.py).  NHWC fp32 activations, HWIO fp32 weights, fp32 MFMA with exact fp32 products.  Any
 * spatial size; padding the TensorFlow way: VALID -> out = (in - k) / s + 1; SAME -> out = ceil(in / s), pad_before =
 * max((out - 1) * s + k - in, 0) / 2.  None of these calls needs a workspace.
 */
typedef struct otgan_incep_conv_desc {
  int N, H, W;     /* batch, input spatial size */
  int C, ldx;      /* input channels, channel stride of the input buffer (>= C) */
  int KH, KW;      /* taps */
  int stride_h, stride_w;
  int same;        /* 1: TF 'SAME' padding, 0: 'VALID' */
  int Cout;        /* output channels, a multiple of 4 */
  int ldy, y_coff; /* output written at channel offset y_coff of a buffer with channel stride ldy */
  int relu;        /* 1: y = max(conv + bias, 0) */
} otgan_incep_conv_desc;

#define OTGAN_INCEP_POOL_MAX 0
#define OTGAN_INCEP_POOL_AVG 1 /* divides by the number of in-bounds taps (TF) */
typedef struct otgan_incep_pool_desc {
  int N, H, W, C, ldx;
  int KH, KW, stride_h, stride_w, same;
  int op;          /* OTGAN_INCEP_POOL_* */
  int ldy, y_coff;
} otgan_incep_pool_desc;

/* output size of one spatial dimension (-1 for bad arguments) */
int otgan_incep_out_size(int in, int k, int stride, int same);
/* y[n, oh, ow, y_coff + co] = act(bias[co] + sum x[n, ih, iw, ci] w[kh][kw][ci][co]); bias nullable; w 16-byte aligned */
int otgan_incep_conv2d_f32(const otgan_incep_conv_desc* d, const float* x, const float* w, const float* bias, float* y,
                           void* stream);
int otgan_incep_pool_f32(const otgan_incep_pool_desc* d, const float* x, float* y, void* stream);
/* y [N, OH, OW, C] (dense) = scale * bilinear(x [N, H, W, C]) + shift; TF's legacy mapping (no half-pixel offset):
 * src = dst * in / out, or dst * (in - 1) / (out - 1) with align_corners; upper neighbour clamped to the edge */
int otgan_incep_resize_f32(int N, int H, int W, int C, int OH, int OW, int align_corners, float scale, float shift,
                           const float* x, float* y, void* stream);
/* pool3 [N, C] = mean of the HW pixels of x (channel stride ldx); logits [N, classes] = pool3 . w (w: [C][classes],
 * no bias); probs = row softmax of logits.  C and classes multiples of 4, pool3 16-byte aligned. */
int otgan_incep_head_f32(int N, int HW, int C, int ldx, int classes, const float* x, const float* w, float* pool3,
                         float* logits, float* probs, void* stream);

/*
 * Feature moments of the Frechet Inception Distance (utils/fid.py), fp64 MFMA, in place:
 *   sum[i] += sum_k x[k][i],  outer[i][j] += sum_k x[k][i] * x[k][j]   for the n rows of x.
 * x: fp32 [n][C] with row stride ldx >= C (pool3 of otgan_incep_head_f32, or a column slice of a wider buffer); sum [C]
 * and outer [C][C] fp64.  Any n >= 0 (n == 0 is a no-op), any C % 4 == 0.  The fp32 inputs are converted to fp64 before
 * the multiply, so every product is exact and only the summation over the rows rounds.  Only elements on or above the
 * diagonal of outer are read; each is computed once and stored to [i][j] and [j][i], so outer is exactly symmetric.
 * Deterministic: the same sequence of calls gives the same bits (no atomics, fixed row order).  No workspace.
 */
int otgan_moments_update_f64(int n, int C, int ldx, const float* x, double* sum, double* outer, void* stream);

/*
 * Kernel sums of the Kernel Inception Distance (utils/kid.py), fp64 MFMA, all subsets in one call.  For subset s with
 * X_i = x[xi[s][i]], Y_j = y[yi[s][j]] (i, j < m) and k(a, b) = (a . b / C + 1)^3:
 *   out[s][0] = sum_{i != j} k(X_i, X_j),   out[s][1] = sum_{i != j} k(Y_i, Y_j),   out[s][2] = sum_{i, j} k(X_i, Y_j).
 * x, y: fp32 rows of C channels with row strides ldx, ldy >= C (pool3 of otgan_incep_head_f32, or a column slice of a wider
 * buffer), 16-byte aligned with strides that are multiples of 4; xi, yi: int32 [nsub][m] row numbers into x and y -- NOT
 * validated here, the caller makes them and checks them; out: double [nsub][3], OVERWRITTEN.  i != j is by position in the
 * list: a row number that occurs twice counts as two rows.  Any m >= 2, any C % 4 == 0, nsub <= 65535 (nsub == 0 launches
 * nothing).  The fp32 inputs are converted to fp64 before the multiply, so every product is exact; the affine map, the cube
 * and all sums are fp64.  No Gram matrix is written: 64 x 64 blocks (only those on or above the diagonal of the two symmetric
 * Grams) are reduced in registers to one double each in `workspace` (otgan_kid_workspace_bytes(nsub, m) bytes, 8-byte
 * aligned) and a second launch adds them per subset in a fixed order.  Deterministic (no atomics): the same call gives the
 * same bits, and a subset's value does not depend on the other subsets of the call.  An argument error returns nonzero
 * without touching out.
 */
size_t otgan_kid_workspace_bytes(int nsub, int m);
int otgan_kid_sums_f64(int nsub, int m, int C, const float* x, int ldx, const int32_t* xi, const float* y, int ldy,
                       const int32_t* yi, double* out, void* workspace, size_t workspace_bytes, void* stream);

/*
 * Nearest-neighbour passes of precision / recall / density / coverage (utils/pr.py; the improved precision and recall of
 * the guided-diffusion evaluator, evaluations/evaluator.py ManifoldEstimator, and prdc's compute_prdc), fp64 MFMA, the
 * distance matrix never written.  With d2(a, b) = max(0, (a.a + b.b) - 2 a.b), for every query row i < nq over the
 * columns j < ny with j != self0 + i (self0 = -1: no column is excluded):
 *   nearest[i][0 .. k) = the k smallest d2(q_i, y_j), ascending; +inf where fewer than k columns were counted,
 *   inside[i]          = #{ j : d2(q_i, y_j) <= thresh[j] }.
 * q, y: fp32 rows of C channels with row strides ldq, ldy >= C, 16-byte aligned with strides that are multiples of 4 (the
 * rules of otgan_kid_sums_f64); thresh: double [ny]; nearest: double [nq][k]; inside: int32 [nq]; both OVERWRITTEN.
 * 0 <= k <= 8, nearest may be null with k == 0; thresh and inside are both null or both given (with ny == 0 there is no
 * threshold to point at and thresh may be null beside an inside, which becomes 0).  The exclusion is by
 * POSITION: another row with the same values is a neighbour at distance 0.  The fp32 inputs are converted to fp64 before
 * the multiply, every dot product -- the norms among them -- adds its channels in an order that depends on C only, so
 * d2(a, b) and d2(b, a) are the same bits in any call, tile or operand role and d2(a, a) == 0.  A k-smallest list and a
 * count are order-free, so the outputs do not depend on the order of the columns, on a row's place in the call or on how
 * the columns are split over workgroups; no atomics.  workspace: otgan_knn_workspace_bytes(nq, ny, k) bytes, 8-byte
 * aligned -- the norms of q and y and k doubles + one count per (column split, query row); OTGAN_ERR_WORKSPACE when
 * smaller.  nq == 0 or ny == 0 returns OTGAN_OK (ny == 0: nearest = +inf, inside = 0).  An argument error returns
 * nonzero without touching the outputs.
 */
size_t otgan_knn_workspace_bytes(int nq, int ny, int k);
int otgan_knn_f64(int nq, int ny, int C, const float* q, int ldq, const float* y, int ldy, int k, int self0,
                  const double* thresh, double* nearest, int32_t* inside, void* workspace, size_t workspace_bytes,
                  void* stream);

/*
 * Nearest neighbours BY IDENTITY, for the k-NN probe of the critic's features (utils/probe.py), fp64 MFMA, the Gram
 * matrix never written.  With s(a, b) = a . b, for every query row i < nq over the columns j < ny with j != self0 + i
 * (self0 = -1: no column is excluded, as in otgan_knn_f64):
 *   index[i][0 .. k) = the columns of the k largest s(q_i, y_j),
 *   score[i][0 .. k) = those values (score may be null),
 * sorted by score descending, equal scores by the SMALLER COLUMN first: a total order, so the outputs are a function of
 * the inputs alone -- not of the order in which columns are visited, of a row's place in the call or of how the columns
 * are split over workgroups; no atomics.  Slots beyond the number of counted columns hold index -1 and score -inf; a
 * counted column, however negative its score, is never displaced by one.
 * q, y: fp32 rows of C channels with row strides ldq, ldy >= C, 16-byte aligned with strides that are multiples of 4,
 * C % 4 == 0 (the rules of otgan_knn_f64); index: int32 [nq][k]; score: double [nq][k]; both OVERWRITTEN.  1 <= k <= 8.
 * The exclusion is by POSITION: another row with the same values is returned, with the score s(a, a).  The fp32 inputs
 * are converted to fp64 before the multiply, and every dot product adds its channels in the order of the one loop that
 * otgan_knn_f64 and otgan_kid_sums_f64 run, which depends on C only: s(a, b) and s(b, a) are the same bits in any
 * call, tile or operand role.  workspace: otgan_topk_dot_workspace_bytes(nq, ny, k) bytes, 8-byte aligned -- k doubles
 * and k int32 per (column split, query row); OTGAN_ERR_WORKSPACE when smaller.  nq == 0 returns OTGAN_OK; ny == 0 fills
 * every slot with -1 and -inf (no workspace needed).  An argument error returns nonzero without touching the outputs.
 * The inputs must be FINITE: a NaN score (a NaN or infinite input row) compares false with everything, so such a column is
 * never listed and its row may report fewer than k neighbours; nothing checks for it.  Column numbers are int32 with
 * 2^31 - 1 reserved for an empty slot, which ny as an int can never reach.
 */
size_t otgan_topk_dot_workspace_bytes(int nq, int ny, int k);
int otgan_topk_dot_f64(int nq, int ny, int C, const float* q, int ldq, const float* y, int ldy, int k, int self0,
                       int32_t* index, double* score, void* workspace, size_t workspace_bytes, void* stream);

/*
 * Exact nearest neighbours of uint8 rows (images in pixel space) BY IDENTITY, for the authenticity score
 * (utils/authenticity.py), on the int8 matrix pipe (csrc/pixnn.hip); the distance matrix is never written.  With
 * d(a, b) = sum_d (a_d - b_d)^2 over the raw uint8 values, for every query row i < nq over the columns j < ny with
 * j != self0 + i (self0 = -1: no column is excluded):
 *   index[i][0 .. k) = the columns of the k smallest d(q_i, y_j),
 *   dist[i][0 .. k)  = those values,
 * sorted by distance ascending, equal distances by the SMALLER COLUMN first: a total order, and every distance is an exact
 * integer, so the outputs are a function of the inputs alone, bit for bit -- not of the order in which columns are
 * visited, of a row's place in the call or of how the columns are split over workgroups; no atomics, no tolerance.  Slots
 * beyond the number of counted columns hold index -1 and dist -1.  The exclusion is by POSITION: another row with the
 * same values is returned, with distance 0 (also when self0 + i >= ny: nothing is excluded then).
 * q, y: uint8 rows of D values with row strides ldq, ldy >= D in bytes, multiples of 16, row pointers 16-byte aligned;
 * D % 16 == 0, 16 <= D <= 49152 (128 x 128 x 3); 1 <= k <= 8; 0 <= ny <= 2^31 - 2; index: int32 [nq][k], dist: int64
 * [nq][k], both OVERWRITTEN.
 * Arithmetic and its bounds: each byte x enters the product as the int8 x - 128 (x ^ 0x80), a common shift that changes no
 * difference, and d = |a|^2 + |b|^2 - 2 a.b with a.b from v_mfma_i32_16x16x64_i8 and the norms from a pre-pass.
 *   |a.b| and the norms are at most D 2^14 <= 49152 x 16384 = 805 306 368 < 2^31: every int32 partial sum is exact;
 *   d is at most D 255^2 = 3 196 108 800 at D = 49152: it does NOT fit int32 and does fit uint32.  The three terms are added
 *   in unsigned 32 bits (the true value is in range, so the wrapped sum is the value) and ordered as the 64-bit key
 *   (d << 32) | j, whose plain unsigned order is the pair order above; the key 2^64 - 1 marks an empty slot, above every
 *   real key.  dist leaves as int64.
 * workspace: otgan_nn_u8_workspace_bytes(nq, ny, k) bytes, 8-byte aligned -- 8 splits nq k bytes of keys (k per column
 * split and query row), then 4 (nq + ny) bytes of norms rounded up to 8; OTGAN_ERR_WORKSPACE when smaller.  nq == 0
 * returns OTGAN_OK; ny == 0 fills every slot with (-1, -1) (no workspace needed).  An argument error returns
 * OTGAN_ERR_INVALID without touching the outputs.
 */
size_t otgan_nn_u8_workspace_bytes(int nq, int ny, int k);
int otgan_nn_u8(int nq, int ny, int D, const uint8_t* q, long ldq, const uint8_t* y, long ldy, int k, int self0,
                int32_t* index, int64_t* dist, void* workspace, size_t workspace_bytes, void* stream);

/*
 * The training batch from a device-resident uint8 dataset in ONE launch (csrc/data.hip; utils/data.py): gather by the
 * epoch's permutation, per-image horizontal flip, uint8 -> [-1, 1] and an optional integer box-downsample -- what the
 * reference does on the host per step (train.py:158,163-170,209-211).
 *   store: NHWC uint8 [n_images][SH][SW][3] (device, 4-byte aligned);  out: fp32 [n_shards * B][S][S][3] with row pitch
 *   ldo >= 3 S S floats, ldo % 4 == 0, 16-byte aligned.  For output row r = s * B + k:
 *     idx = perm ? perm[shard_offsets[s] + k] : shard_offsets[s] + k      (perm: device int32 [perm_len], nullable; its
 *                                                                          VALUES are the caller's to validate: 0 <= . < n_images)
 *     xs  = flip && flip[r] ? S - 1 - x : x                               (flip: device uint8 [n_shards * B], nullable)
 *     f = SH / S = SW / S in {1, 2, 4}, S % 4 == 0
 *     f == 1: out[r][y][x][c] = lut[store[idx][y][xs][c]]                 (lut: 256 device floats; the host passes
 *             arange(256) / 127.5 - 1 in fp32, the expression of the host loader: the same bits by construction)
 *     f > 1:  out[r][y][x][c] = (float)sum / (127.5f * f * f) - 1.0f, sum = the exact integer sum of the f x f box of channel
 *             c at (f y, f xs)                                            (lut unused)
 *   shard_offsets: HOST array of n_shards <= OTGAN_BATCH_U8_MAX_SHARDS entries (it travels in the kernel arguments); every
 *   shard must lie inside the permutation (the store without one): shard_offsets[s] + B <= perm_len (n_images).
 * All byte offsets are 64-bit.  Enqueues exactly one kernel on `stream`: no allocation, no copy, no synchronisation.
 */
#define OTGAN_BATCH_U8_MAX_SHARDS 32
int otgan_batch_from_u8_f32(const uint8_t* store, long n_images, int SH, int SW, const int32_t* perm, long perm_len,
                            const long* shard_offsets, int n_shards, int B, const uint8_t* flip, const float* lut, int S,
                            float* out, long ldo, void* stream);

/*
 * Differentiable augmentation of the critic's inputs (Zhao et al. 2020, "DiffAugment"; csrc/augment.hip, utils/augment.py):
 * y = T(x) per image, T = cutout o translation o colour with parameters derived ON THE DEVICE from the image's row of
 * uniforms, and dx = T^T dy, the exact transpose (T is affine in x: the brightness offset has no transpose term).
 *   x, y, dy, dx: fp32 NHWC [rows][S][S][3], contiguous, 16-byte aligned, output distinct from input; S % 4 == 0, 4 <= S <= 64.
 *   u: device fp32 [rows][8], uniforms in [0, 1); slot 7 is unused.
 *   policy: OTGAN_AUG_COLOR | OTGAN_AUG_TRANSLATION | OTGAN_AUG_CUTOUT; a group whose bit is off is the identity and its slots
 *   are not read as parameters.  Policy 0 is a plain copy.
 * Parameters of image r from u[r] (fp32 arithmetic, every float -> int by truncation):
 *   colour:       b = u0 - 0.5f,  ks = 2 u1,  kc = u2 + 0.5f
 *   translation:  R = (S + 4) / 8 (4 at 32, 8 at 64);  tx = min((int)(u3 (2R + 1)), 2R) - R,  ty likewise from u4
 *   cutout:       c = S / 2;  ox = min((int)(u5 (S + 1)), S),  oy likewise from u6;  the window is
 *                 [ox - c/2, ox + c/2) x [oy - c/2, oy + c/2) (columns x rows) intersected with the image
 * Forward, output pixel (yy, xx), channel ch:
 *   +0.0f                              if (yy, xx) lies in the cutout window,
 *   +0.0f                              else if the source pixel (yy - ty, xx - tx) is outside the image,
 *   colour(x[r][yy - ty][xx - tx])[ch] else, where for a pixel v = (v_R, v_G, v_B)
 *     v1 = v + b;   m = (v1_R + v1_G + v1_B) / 3;   v2 = (v1 - m) ks + m;
 *     mu = (sum of all 3 S^2 elements of x[r]) / (3 S^2) + b;   v3 = (v2 - mu) kc + mu = colour(v).
 *   Without OTGAN_AUG_COLOR colour() is not evaluated: a copied element has the bits of its source.
 * Backward:
 *   e[q]  = dy[q + t] where the output position q + t = (y + ty, x + tx) is inside the image and outside the window, else 0;
 *   e2    = kc e + (1 - kc) mean_image(e)            (mean over the 3 S^2 elements of the image)
 *   dx    = ks e2 + (1 - ks) mean_channels(e2)       (mean over the 3 channels of the pixel);   dx = e without OTGAN_AUG_COLOR.
 * Deterministic and position-independent: one workgroup per image; both per-image sums run in a fixed order that depends on S
 * only (a fixed sequence per thread, a wave butterfly, a fixed tree over the waves; no atomics, nothing crosses a workgroup),
 * so an image's output bits depend on its pixels, its row of u, S and policy -- not on rows, its row index or the call.
 * Each entry point enqueues exactly one kernel on `stream` (none for rows == 0): no allocation, no copy, no synchronisation.
 * A null pointer, rows < 0, an unsupported S, a policy outside the mask or a misaligned pointer returns OTGAN_ERR_INVALID
 * with a message before any launch.
 */
#define OTGAN_AUG_COLOR 1
#define OTGAN_AUG_TRANSLATION 2
#define OTGAN_AUG_CUTOUT 4
int otgan_augment_fwd_f32(const float* x, long rows, int S, const float* u, int policy, float* y, void* stream);
int otgan_augment_bwd_f32(const float* dy, long rows, int S, const float* u, int policy, float* dx, void* stream);

/*
 * The sliced Wasserstein distance on Laplacian-pyramid patches (Karras et al. 2018, "Progressive Growing of GANs", section 5;
 * csrc/swd.hip, utils/swd.py): the device stages between two sets of uint8 images and the per-direction sorts.  The descriptor
 * matrix (n P x 147 floats per level and set) is never written.
 *   img: NHWC uint8 [n][S][S][3], contiguous, 4-byte aligned.  S in {16, 32, 64}; any other S returns OTGAN_ERR_UNSUPPORTED.
 *   Levels: L = log2(S / 16) + 1 = otgan_swd_levels(S) (0 for an unsupported S); level l has side S_l = S >> l, the last is 16 x 16.
 * Pyramid of one image, per channel, in fp32:
 *   g = [1 4 6 4 1] (x) [1 4 6 4 1] / 256;  border = mirror WITHOUT repeating the edge pixel (index -1 -> 1, s -> s - 2:
 *   scipy.ndimage's mode='mirror');  down(x) = (g * x)[::2, ::2];  up(x) = (4 g) * z with z = x on the even pixels of a zero
 *   image of twice the side.
 *   pyr[0] = float(img);  for i = 1 ... L - 1:  pyr[i] = down(pyr[i - 1]),  then  pyr[i - 1] -= up(pyr[i]).  The last level stays
 *   Gaussian.  A 5 x 5 sum is taken with the integer weights in the order dy outer, dx inner and scaled once; with uint8 inputs
 *   every stage but up() of the 16 x 16 level at S = 64 is exact in fp32.
 * otgan_swd_pyramid_u8: out fp32 [n][S_l][S_l][3] (16-byte aligned) = level `level` of every image.  A staged entry for tests.
 * Descriptors: pos int32 [L][n][P][2] (device) holds the top-left (y, x) of P patches of 7 x 7 x 3 per image and level,
 *   0 <= y, x <= S_l - 7 (the caller's to guarantee; a value outside is moved to the nearest bound, so nothing is read out of
 *   bounds).  A descriptor is the patch flattened in [channel][dy][dx] order: 147 values, element e = (c 7 + dy) 7 + dx.
 * otgan_swd_channel_stats_u8: for every level l and channel c, over ALL n P 49 descriptor elements of that channel,
 *   mean[l][c] = sum x / N,   inv_std[l][c] = 1 / sqrt(sum x^2 / N - mean^2)   (population std, ddof = 0; fp64, stored as fp32
 *   [L][3]).  A zero variance gives +inf -- and NaN projections, loud.  The statistics are those of the EXACT pyramid (built in
 *   fp64 here; the fp32 pyramid's one inexact stage would show in the near-zero mean of a Laplacian level).  Per image the sums
 *   are taken in fp64 in a fixed order;
 *   across images they are added EXACTLY (every level value is a multiple of 2^-22, so the per-image sums scale to integers that
 *   are added in int64): the outputs do not depend on the order of the images.  n >= 1, n P <= 2^27.  Two launches on `stream`,
 *   no atomics, no host synchronisation.  workspace: otgan_swd_workspace_bytes(n, S, P) bytes, 8-byte aligned (the per-image
 *   sums); OTGAN_ERR_WORKSPACE when smaller.
 * otgan_swd_project_u8: for level `level`, every direction j < nd, image i < n and patch p < P
 *   proj[j][i P + p] = sum over e of ((x_e - mean[level][c_e]) inv_std[level][c_e]) dirs[j][e]
 *   with dirs fp32 [nd][147] and proj fp32 [nd][ldp], ldp >= n P; columns >= n P are not touched.  fp32, one fma per element in
 *   the order e = 0 ... 146: the bits of an output depend on the image, its positions, mean, inv_std and dirs[j] alone -- not on
 *   n, nd, or which images and directions share a call (a caller that splits the images passes each part's own pos [L][n'][P][2]
 *   and proj + i0 P).  One launch; nd == 0 or n == 0 returns OTGAN_OK without one.
 * otgan_swd_row_l1_f64: out[r] = (sum over k < m of |a[r][k] - b[r][k]|) / m for r < rows, a and b fp32 with row strides
 *   lda, ldb >= m, converted to fp64 before the subtraction; a fixed summation order per row that depends on m only.
 * An argument error returns nonzero with a message before any launch.
 */
int otgan_swd_levels(int S);
int otgan_swd_pyramid_u8(const uint8_t* img, long n, int S, int level, float* out, void* stream);
size_t otgan_swd_workspace_bytes(long n, int S, int P);
int otgan_swd_channel_stats_u8(const uint8_t* img, long n, int S, const int32_t* pos, int P, float* mean, float* inv_std,
                               void* workspace, size_t workspace_bytes, void* stream);
int otgan_swd_project_u8(const uint8_t* img, long n, int S, const int32_t* pos, int P, int level, const float* mean,
                         const float* inv_std, const float* dirs, int nd, float* proj, long ldp, void* stream);
int otgan_swd_row_l1_f64(const float* a, long lda, const float* b, long ldb, int rows, long m, double* out, void* stream);

/* ---------------------------------------------------------------------------------------
 * Health of a training step (--health_every; utils/health.py; csrc/health.hip): gradient, parameter and update statistics of
 * every variable in one pass, and the marginal residuals of Sinkhorn plans.  Nothing the reference computes.
 *
 * otgan_tensor_health_f32: nseg tensors ("segments") in one call.  x and ref are HOST arrays of nseg DEVICE pointers (fp32,
 *   4-byte aligned, any alignment beyond that), as otgan_cost_matrix_batched_f32 takes them; ref, or any of its entries, may be
 *   null; n is a HOST array of element counts, 0 allowed (x[i] is then not read and may be null).  Any nseg >= 0: segments go out
 *   in launches of OTGAN_HEALTH_MAX_SEGMENTS.
 *   out: double [nseg][6] (device), per segment, over the FINITE elements of x (a non-finite x_k enters none of slots 0 - 4):
 *     0  sum x^2          1  max |x|
 *     2  sum (x - ref)^2  3  max |x - ref|      over the elements where ref is finite too; both 0 when ref is null
 *     4  the count of exact zeros (+0 and -0)   5  the count of non-finite elements (inf, NaN) of x
 *   hist: unsigned 64-bit [nseg][256] (device), per segment one count per finite non-zero element, in the bucket of its biased
 *     fp32 exponent (bits 30 ... 23 of |x|): denormals in bucket 0, bucket 255 stays empty.  sum(hist) + out[4] + out[5] == n.
 *   Arithmetic: x^2 is exact in fp64; d = (double)x - (double)ref and d * d are one IEEE fp64 operation each; the sums are fp64
 *   in a fixed order: a segment is cut into chunks of OTGAN_HEALTH_CHUNK elements counted from its own first element, a chunk is
 *   summed as thread t of 256 = elements t, t + 256, ... in order, then a 64-lane butterfly, then the four wave sums as
 *   (w0 + w1) + (w2 + w3); the chunks' partial results go to the workspace and a finishing launch adds them the same way.  No
 *   float atomics (the histogram uses integer adds).  A segment's 6 + 256 numbers are therefore the same bits alone or among
 *   other segments, at any pointer alignment, and from call to call.  One pass over x and ref: 16-byte loads on the 16-byte
 *   aligned body of a chunk, scalar loads on its head and tail.
 *   workspace: otgan_tensor_health_workspace_bytes(n, nseg) bytes, 8-byte aligned; OTGAN_ERR_WORKSPACE when smaller.
 *
 * otgan_plan_marginals_f32: plan fp32 [P][n][ldp] (ldp >= m; rectangular and pitched plans) -> out double [P][4] (device):
 *     0  max_i |r_i - 1|   1  mean_i |r_i - 1|   2  max_j |c_j - n/m|   3  mean_j |c_j - n/m|
 *   with r_i = sum_j plan[p][i][j] and c_j = sum_i plan[p][i][j] taken in fp64 in a fixed order that depends on (n, m) only; no
 *   atomics.  n, m >= 1.  workspace: otgan_plan_marginals_workspace_bytes(P, n, m) bytes, 8-byte aligned.
 * An argument error returns nonzero with a message before any launch.
 */
#define OTGAN_HEALTH_CHUNK 2048
#define OTGAN_HEALTH_MAX_SEGMENTS 64
size_t otgan_tensor_health_workspace_bytes(const long* n, int nseg);
int otgan_tensor_health_f32(const float* const* x, const float* const* ref, const long* n, int nseg, double* out,
                            unsigned long long* hist, void* workspace, size_t workspace_bytes, void* stream);
size_t otgan_plan_marginals_workspace_bytes(int P, int n, int m);
int otgan_plan_marginals_f32(const float* plan, int P, int n, int m, long ldp, double* out, void* workspace,
                             size_t workspace_bytes, void* stream);

#endif /* OTGAN_LAYERS_H */
