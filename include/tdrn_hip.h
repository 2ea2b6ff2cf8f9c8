/*
 * tdrn_hip.h -- C ABI of libtdrn_hip.so: the MI355X (gfx950) inference path of TDRN's
 * dual-refinement detector.  Plain pointers and sizes only (no torch / THC types).
 *
 * Conventions:
 *   - return 0 (TDRN_OK) on success; NEGATIVE = argument / shape error (the reference's
 *     shape_check / THArgCheck cases); POSITIVE = hipError_t of a failed HIP call.  Nothing
 *     is printf'ed-and-ignored (the reference does: deform_conv_cuda_kernel.cu:233-237,
 *     nms_kernel.cu:12-19).
 *   - every device buffer is owned by the caller (PyTorch-ROCm allocates them); functions that
 *     need scratch take a (workspace, workspace_bytes) pair sized by the matching
 *     *_workspace_bytes() query.  No hipMalloc / hipFree / device sync inside the hot calls
 *     (so they can be captured into a hipGraph); the two exceptions are marked COMPAT.
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream); all work is
 *     enqueued on it and the call returns without synchronising unless stated.
 *   - thread-safe per (handle, stream).  The only process-wide state is idempotent memoisation: environment
 *     switches (TDRN_*) read once, and "dynamic LDS limit raised" per (kernel, device).
 *
 * Each entry point cites the reference interface it replaces (paths relative to the upstream
 * SeanChenxy/TDRN tree).
 */
#ifndef TDRN_HIP_H
#define TDRN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TDRN_API __attribute__((visibility("default")))

/* ---- status codes ---------------------------------------------------------------------- */
#define TDRN_OK 0
#define TDRN_E_ARG (-1)          /* null pointer / bad enum / bad size                          */
#define TDRN_E_SHAPE (-2)        /* shape_check failure (deform_conv_cuda.c:7-96)               */
#define TDRN_E_WORKSPACE (-3)    /* workspace too small                                         */
#define TDRN_E_UNSUPPORTED (-4)  /* configuration outside what the kernels cover                */
#define TDRN_E_PARAM (-5)        /* unknown / missing / mis-shaped state_dict entry             */
#define TDRN_E_STATE (-6)        /* call order (e.g. forward before weights were packed)        */
#define TDRN_E_VALUE (-7)        /* Detect: nms_thresh <= 0 (layers/functions/detection.py:20)  */
#define TDRN_E_DEVICE (-8)       /* a device-side hand-off of an earlier forward timed out: its outputs are invalid (tdrn_net_check) */

TDRN_API const char *tdrn_version(void);
TDRN_API const char *tdrn_error_string(int code);

/* arithmetic type of the dense path (activations + weights in HBM, MFMA input type);
 * accumulation is always fp32; box decoding / NMS / offsets / bilinear weights always fp32. */
typedef enum { TDRN_F32 = 0, TDRN_BF16 = 1, TDRN_F16 = 2 } tdrn_dtype;

/* ========================================================================================
 * (i) Deformable convolution v1 forward -- replaces
 *     int deform_conv_forward_cuda(THCudaTensor *input, *weight, *offset, *output, *columns,
 *         *ones, int kW, int kH, int dW, int dH, int padW, int padH, int dilationH,
 *         int dilationW, int deformable_group)          utils/deformconv/deform_conv_cuda.h:1-7
 *     called from ConvOffset2dFunction.forward          model/networks.py:641-645
 *     kernel semantics                                  utils/deformconv/deform_conv_cuda_kernel.cu:15-51,156-208
 *   input  (N, Cin, H, W)  fp32 NCHW contiguous, device
 *   weight (Cout, Cin, kH, kW) fp32 contiguous, device        (no bias, like the reference)
 *   offset (N, G*2*kH*kW, Ho, Wo) fp32, device
 *   output (N, Cout, Ho, Wo) fp32, device, fully overwritten
 *   `columns` / `ones` of the reference have no counterpart: the sampled columns never leave
 *   LDS.  `compute` selects the MFMA input type (TDRN_F32 reproduces the reference's fp32).
 *   Kernel size, stride, padding and dilation are per axis, as in the reference (any kH x kW).
 *   Shape errors mirror shape_check (deform_conv_cuda.c:7-96, :137) -> TDRN_E_SHAPE.
 * ====================================================================================== */
TDRN_API size_t tdrn_deform_conv_workspace_bytes(int N, int Cin, int H, int W, int Cout, int kH,
                                                 int kW, int dH, int dW, int padH, int padW,
                                                 int dilationH, int dilationW,
                                                 int deformable_group, tdrn_dtype compute);
TDRN_API int tdrn_deform_conv_forward(const float *input, const float *weight,
                                      const float *offset, float *output, int N, int Cin, int H,
                                      int W, int Cout, int kW, int kH, int dW, int dH, int padW,
                                      int padH, int dilationH, int dilationW,
                                      int deformable_group, tdrn_dtype compute, void *workspace,
                                      size_t workspace_bytes, void *stream);

/* ========================================================================================
 * (i-b) Deformable convolution v1 backward, fp32 -- replaces
 *     int deform_conv_backward_input_cuda(THCudaTensor *input, *offset, *gradOutput, *gradInput,
 *         *gradOffset, *weight, *columns, int kW, int kH, int dW, int dH, int padW, int padH,
 *         int dilationH, int dilationW, int deformable_group)      utils/deformconv/deform_conv_cuda.h:9-13
 *     int deform_conv_backward_parameters_cuda(THCudaTensor *input, *offset, *gradOutput,
 *         *gradWeight, *columns, *ones, int kW, ..., int deformable_group, float scale)  :15-19
 *     called from ConvOffset2dFunction.backward         model/networks.py:648-681
 *     kernel semantics                                  utils/deformconv/deform_conv_cuda_kernel.cu:53-154,247-298,337-400
 *   Tensors as in (i); grad_output (N, Cout, Ho, Wo) fp32 NCHW contiguous.  `columns` / `ones` are dropped.
 *   backward_input:       grad_input (N, Cin, H, W) += the input gradient (float atomics: the low bits depend on
 *                         arrival order); grad_offset (N, G*2*kH*kW, Ho, Wo) is OVERWRITTEN (bitwise reproducible).
 *   backward_parameters:  grad_weight (Cout, Cin, kH, kW) += scale * grad_output . columns^T, summed in a fixed order
 *                         (bitwise reproducible).
 *   The sampling rule is the forward's: a coordinate < 0 or >= H (W) contributes nothing; in [H-1, H) all of the weight
 *   goes to row H-1 and the offset gradient along that axis is 0; at an exact integer the offset gradient is the one-sided
 *   v_high - v_low.  One workspace query serves both entries; it returns 0 where the forward's query does (shape_check),
 *   and the entries then return TDRN_E_SHAPE (TDRN_E_UNSUPPORTED beyond the kernels' LDS budget: Cout above ~2000).
 *   No allocation and no host synchronisation: everything is enqueued on `stream`.
 * ====================================================================================== */
TDRN_API size_t tdrn_deform_conv_backward_workspace_bytes(int N, int Cin, int H, int W, int Cout, int kH, int kW,
                                                          int dH, int dW, int padH, int padW, int dilationH,
                                                          int dilationW, int deformable_group);
TDRN_API int tdrn_deform_conv_backward_input(const float *input, const float *offset, const float *grad_output,
                                             float *grad_input, float *grad_offset, const float *weight, int N,
                                             int Cin, int H, int W, int Cout, int kW, int kH, int dW, int dH,
                                             int padW, int padH, int dilationH, int dilationW,
                                             int deformable_group, void *workspace, size_t workspace_bytes,
                                             void *stream);
TDRN_API int tdrn_deform_conv_backward_parameters(const float *input, const float *offset, const float *grad_output,
                                                  float *grad_weight, int N, int Cin, int H, int W, int Cout, int kW,
                                                  int kH, int dW, int dH, int padW, int padH, int dilationH,
                                                  int dilationW, int deformable_group, float scale,
                                                  void *workspace, size_t workspace_bytes, void *stream);

/* ========================================================================================
 * (i-c) Dense conv2d with gradients -- what nn.Conv2d + autograd give the reference's training loop (train.py; the
 *     dense layers of model/dualrefinedet_vggbn.py:30-117): forward, input gradient, weight / bias gradient.
 *   input (N, Cin, H, W), weight (Cout, Cin, kH, kW) OIHW, bias (Cout) or NULL, output / grad_output (N, Cout, Ho, Wo),
 *   grad_input like input, grad_weight like weight, grad_bias (Cout) or NULL: all fp32, contiguous, device.
 *   `compute` selects the MFMA input type as in (i): TDRN_F32 is exact fp32; TDRN_BF16 / TDRN_F16 round input, weight and
 *   grad_output ONCE, to nearest even, to the type (bias is not rounded).  Accumulation and every output are fp32.
 *   At the ends of the range that rounding keeps the type's subnormals (nothing is flushed, neither by the packers nor as an MFMA
 *   operand), turns a value past the largest finite one into +-inf (65520 is the first in fp16; nothing saturates) and leaves NaN a
 *   NaN; in TDRN_F32 compute fp32 subnormals are kept as operands, in the accumulation and in every output.  A non-finite operand
 *   meets the zeros of the other operand as IEEE says (inf * 0 = NaN), and the padding is explicit zeros: a non-finite weight at a
 *   tap that reaches into the padding gives NaN there, as a non-finite value gives NaN under a zero weight
 *   (tests/test_gpu_number_range.py measures all of this, bit for bit).
 *   forward:             output is OVERWRITTEN.
 *   backward_input:      grad_input is OVERWRITTEN (a stride-1 conv over grad_output with the kernel rotated and transposed).
 *   backward_parameters: grad_weight += scale * sum_p grad_output[p] input[p (+) tap], grad_bias += scale * sum_p grad_output[p],
 *                        split over K = N*Ho*Wo and summed in a fixed order.
 *   All gradients are bitwise reproducible run to run: nothing on this path uses float atomics, and the split count depends
 *   on the geometry alone.
 *   Geometry (the argument order is the query's in all four functions): square kernels kH = kW in {1, 3}, stride 1,
 *   dilationH = dilationW >= 1, 0 <= padH = padW <= dilation * (k - 1), groups = 1.
 *   Errors, all decided before any launch: a null pointer -> TDRN_E_ARG; k <= 0, stride / dilation <= 0, negative pad,
 *   N / Cin / Cout / H / W <= 0, an output smaller than 1 x 1 -> query 0 and TDRN_E_SHAPE; well-formed geometry outside the
 *   list above (stride != 1, other kernel sizes, pad > dilation * (k - 1), per-axis pad / dilation, N*H*W*Cin_pad or
 *   N*Ho*Wo*Cout_pad of 2^31 elements or more, channels padded to 64) -> query 0 and TDRN_E_UNSUPPORTED; a workspace below the
 *   query -> TDRN_E_WORKSPACE.  One query serves all three entries.  No allocation and no host synchronisation: everything is
 *   enqueued on `stream`.
 * ====================================================================================== */
TDRN_API size_t tdrn_conv2d_workspace_bytes(int N, int Cin, int H, int W, int Cout, int kH, int kW, int dH, int dW, int padH,
                                            int padW, int dilationH, int dilationW, tdrn_dtype compute);
TDRN_API int tdrn_conv2d_forward(const float *input, const float *weight, const float *bias, float *output, int N, int Cin,
                                 int H, int W, int Cout, int kH, int kW, int dH, int dW, int padH, int padW, int dilationH,
                                 int dilationW, tdrn_dtype compute, void *workspace, size_t workspace_bytes, void *stream);
TDRN_API int tdrn_conv2d_backward_input(const float *grad_output, const float *weight, float *grad_input, int N, int Cin,
                                        int H, int W, int Cout, int kH, int kW, int dH, int dW, int padH, int padW,
                                        int dilationH, int dilationW, tdrn_dtype compute, void *workspace,
                                        size_t workspace_bytes, void *stream);
TDRN_API int tdrn_conv2d_backward_parameters(const float *input, const float *grad_output, float *grad_weight,
                                             float *grad_bias, int N, int Cin, int H, int W, int Cout, int kH, int kW, int dH,
                                             int dW, int padH, int padW, int dilationH, int dilationW, float scale,
                                             tdrn_dtype compute, void *workspace, size_t workspace_bytes, void *stream);

/* ========================================================================================
 * (i-d) BatchNorm2d with an optional fused ReLU, forward and backward -- what nn.BatchNorm2d + nn.ReLU + autograd give the
 *     reference's training loop (the fifteen pairs of model/dualrefinedet_vggbn.py; vgg(), model/networks.py:136-163).
 *   input / output / grad_output / grad_input (N, C, H, W); weight, bias, running_mean, running_var, save_mean, save_invstd,
 *   grad_weight, grad_bias (C): all fp32, contiguous, device, on any 4-byte boundary.  M = N*H*W values per channel.
 *   forward, training = 1: mean and biased variance of the batch (chunked Welford records merged with Chan's formula, never
 *                        E[x^2] - E[x]^2) -> save_mean, save_invstd = 1 / sqrt(var + eps); running_mean = (1 - momentum) running_mean +
 *                        momentum mean and running_var likewise with the UNBIASED variance M2 / (M - 1), once per call
 *                        (nn.BatchNorm2d's semantics; both NULL: nothing is updated).
 *            training = 0: save_mean = running_mean, save_invstd = 1 / sqrt(running_var + eps); the running buffers are only read.
 *            z = (input - save_mean) (weight save_invstd) + bias; output = relu ? max(z, 0) : z, OVERWRITTEN.
 *   backward: dy' = grad_output [z > 0] with z recomputed from input (relu = 0: dy' = grad_output), xhat = (input - save_mean) save_invstd;
 *            grad_weight += scale sum dy' xhat, grad_bias += scale sum dy' (both or neither; NULL: not computed);
 *            grad_input (NULL: not computed) is OVERWRITTEN with weight save_invstd (dy' - (sum dy' + xhat sum dy' xhat) / M) for
 *            training = 1 and with weight save_invstd dy' for training = 0.  One of grad_input and the pair is required.
 *   A channel's reduction is cut into splits that depend on (N, C, H*W) alone and merged in split order: no float atomics, every
 *   output of both entries is bitwise reproducible, and the same for a buffer on any 4-byte boundary.
 *   The query returns 12 C splits + 8 C bytes and serves both entries.
 *   Range of the batch statistics, per channel (tests/test_gpu_number_range_stats.py; the bounds are derived in
 *   tests/_number_range_stats.py): save_mean is right to a few u max|x| and M2 -- so save_invstd and running_var -- to a relative
 *   c u (1 + |mean| / sigma), u = 2^-24, at any scale of the data and whatever the mean (a merge with an empty record returns the
 *   other record, so a mean past 2^64 is no special case), while M (max x - min x)^2 < 2^128: then no d * d * n of a merge and no
 *   squared deviation overflows.  Squared deviations below 2^-126 are kept at the subnormal spacing and vanish below 2^-150 (M2 = 0
 *   for sigma < 2^-75: save_invstd = 1 / sqrt(eps)).  Past the range M2 is +inf, never NaN, for |x| < 2^123: variance inf ->
 *   save_invstd = 0 -> output = bias (clipped by the ReLU), grad_input = 0 and grad_weight += 0 for that channel, running_var = +inf;
 *   save_mean stays right.  Other channels are not touched.
 *   Errors, all decided before any launch: a null required pointer, a pointer off a 4-byte boundary, grad_weight without grad_bias,
 *   training = 0 without running buffers -> TDRN_E_ARG; N / C / H / W <= 0 -> query 0 and TDRN_E_SHAPE; training = 1 with M = 1 ->
 *   TDRN_E_SHAPE (M = 2 is legal); N*C*H*W >= 2^31 -> query 0 and TDRN_E_UNSUPPORTED; eps <= 0 or momentum outside [0, 1] -> TDRN_E_ARG;
 *   a workspace below the query -> TDRN_E_WORKSPACE.  No allocation and no host synchronisation: everything is enqueued on `stream`.
 * ====================================================================================== */
TDRN_API size_t tdrn_batch_norm_workspace_bytes(int N, int C, int H, int W);
TDRN_API int tdrn_batch_norm_forward(const float *input, const float *weight, const float *bias, float *running_mean,
                                     float *running_var, float *output, float *save_mean, float *save_invstd, int N, int C, int H,
                                     int W, int training, float momentum, float eps, int relu, void *workspace,
                                     size_t workspace_bytes, void *stream);
TDRN_API int tdrn_batch_norm_backward(const float *input, const float *grad_output, const float *weight, const float *bias,
                                      const float *save_mean, const float *save_invstd, float *grad_input, float *grad_weight,
                                      float *grad_bias, int N, int C, int H, int W, int training, int relu, float scale,
                                      void *workspace, size_t workspace_bytes, void *stream);

/* ========================================================================================
 * (i-e) MaxPool2d and L2Norm, forward and backward -- what nn.MaxPool2d, layers/modules/l2norm.py and autograd give the reference's
 *     training loop (the five pools of vgg(), model/networks.py:136-163, and the two L2Norm layers of the source maps).
 *   All tensors fp32, contiguous NCHW, device, on any 4-byte boundary (the code tensor on any byte), fewer than 2^31 elements.
 *   MaxPool2d.  Geometries: kernel 2 / stride 2 / pad 0 with ceil_mode 0 or 1, and kernel 3 / stride 1 / pad 1.  Output size per axis:
 *            floor or ceil of (in + 2 pad - kernel) / stride, plus 1; in ceil mode the last window must start inside the input
 *            (torch's rule).  tdrn_max_pool_output_size returns it, 0 for another geometry or when no window fits.
 *   forward: a window's in-bounds elements are scanned row-major; a value replaces the running maximum when it is strictly greater or
 *            is NaN (torch's rule: the first of equal maxima wins, a NaN wins, the last NaN is the selected element).  output
 *            (N, C, Ho, Wo) is OVERWRITTEN; code (N, C, Ho, Wo) uint8, or NULL for an inference-only forward, gets the selected
 *            element's slot dy * kernel + dx in the unclipped window.
 *   backward: grad_input (N, C, H, W) is OVERWRITTEN, every element exactly once, from grad_output and code alone (the input is not
 *            read): the sum, in window row-major order and starting from +0.0, of grad_output over the windows whose code names the
 *            element.  An element of no window, or selected by none, gets +0.0.
 *   L2Norm.   output = weight[c] input / norm with norm[n, h, w] = sqrt(sum_c input^2) + eps (eps outside the root, the reference's
 *            module), OVERWRITTEN; norm (N, H, W), or NULL, is all the backward needs besides the input.
 *   backward: with r = norm - eps and s = sum_c weight go input per pixel, grad_input (NULL: not computed) is OVERWRITTEN with
 *            weight go / norm - input s / (norm^2 r); at an all-zero pixel (r = 0) the second term is taken as 0 (the function is
 *            weight input / eps there; torch's autograd returns NaN).  grad_weight (NULL: not computed) += scale sum_pixels go input / norm,
 *            summed per 64-pixel tile and over the tiles in tile order.  One of the two is required.  The workspace is needed for
 *            grad_weight only; the query returns 4 C ceil(N H W / 64) bytes, a pure function of (N, C, H W).
 *   Range (tests/test_gpu_number_range_stats.py): the sum of squares is an fp32 sum, so norm is right to (C / 2 + 3) u while
 *            sum_c input^2 < 2^128; a square below 2^-126 is kept at the subnormal spacing and vanishes below 2^-150, which moves norm
 *            by at most sqrt(C 2^-149).  A pixel whose squares all vanish (|input| < 2^-75, subnormals included) has norm = eps and
 *            r = 0 exactly and is treated as the all-zero pixel: output = weight input / eps, grad_input = weight go / eps.  Where
 *            norm is within a few ulp of eps, r = norm - eps carries ulp(norm) / 2 of absolute error and the second term of
 *            grad_input that much relative error over r.  Past 2^128 norm = +inf and output = +-0, as the fp32 formula gives; the
 *            backward gives grad_input = +-0 at that pixel and adds 0 to grad_weight (1 / inf = 0; no NaN while sum_c weight go input
 *            is finite).  Other pixels are not touched, whatever their neighbours' scale.
 *   No float atomics: every output of the four entries is bitwise reproducible, and the same for a buffer on any 4-byte boundary.
 *   Errors, all decided before any launch, in this order: a null required pointer, a float pointer off a 4-byte boundary, eps <= 0
 *   or NaN -> TDRN_E_ARG; N / C / H / W <= 0 or an empty output -> TDRN_E_SHAPE (queries: 0); 2^31 or more elements or a pool
 *   geometry outside the list -> TDRN_E_UNSUPPORTED (queries: 0); grad_weight with a workspace below the query -> TDRN_E_WORKSPACE.
 *   No allocation and no host synchronisation: everything is enqueued on `stream`.
 * ====================================================================================== */
TDRN_API int tdrn_max_pool_output_size(int in, int kernel, int stride, int pad, int ceil_mode);
TDRN_API int tdrn_max_pool_forward(const float *input, float *output, unsigned char *code, int N, int C, int H, int W, int kernel,
                                   int stride, int pad, int ceil_mode, void *stream);
TDRN_API int tdrn_max_pool_backward(const float *grad_output, const unsigned char *code, float *grad_input, int N, int C, int H, int W,
                                    int kernel, int stride, int pad, int ceil_mode, void *stream);
TDRN_API size_t tdrn_l2norm_workspace_bytes(int N, int C, int H, int W);
TDRN_API int tdrn_l2norm_forward(const float *input, const float *weight, float *output, float *norm, int N, int C, int H, int W,
                                 float eps, void *stream);
TDRN_API int tdrn_l2norm_backward(const float *input, const float *grad_output, const float *weight, const float *norm,
                                  float *grad_input, float *grad_weight, int N, int C, int H, int W, float eps, float scale,
                                  void *workspace, size_t workspace_bytes, void *stream);

/* ========================================================================================
 * (i-f) ConvTranspose2d with kernel 2, stride 2 and gradients -- what nn.ConvTranspose2d(256, 256, 2, 2, 0) + autograd give the
 *     reference's training loop (the up_layers of add_refine_head: the TCB pyramid of dualrefinedet_vggbn, dualrefinedet_mobilenet
 *     and refinedet_vgg): forward, input gradient, weight / bias gradient.
 *   input (N, Cin, H, W), weight (Cin, Cout, 2, 2) (torch's layout), bias (Cout) or NULL, output / grad_output (N, Cout, 2H, 2W),
 *   grad_input like input, grad_weight like weight, grad_bias (Cout) or NULL: all fp32, contiguous, device, on any 4-byte boundary.
 *   `compute` as in (i-c): TDRN_BF16 / TDRN_F16 round input, weight and grad_output ONCE, to nearest even (bias is not rounded);
 *   accumulation and every output are fp32.  With kernel 2 at stride 2 every output pixel has exactly one tap:
 *   forward:             output[n][co][2h+i][2w+j] = bias[co] + sum_ci input[n][ci][h][w] weight[ci][co][i][j], OVERWRITTEN.
 *   backward_input:      grad_input[n][ci][h][w] = sum_{i,j,co} grad_output[n][co][2h+i][2w+j] weight[ci][co][i][j], OVERWRITTEN.
 *   backward_parameters: grad_weight[ci][co][i][j] += scale * sum_{n,h,w} input[n][ci][h][w] grad_output[n][co][2h+i][2w+j],
 *                        grad_bias[co] += scale * sum grad_output[.][co][.][.]; split over K = N*H*W and summed in a fixed order.
 *   All outputs are bitwise reproducible run to run, and the same for caller buffers on any 4-byte boundary: nothing on this path
 *   uses float atomics, and the split counts depend on the geometry alone.
 *   Geometry (the argument order is the query's in all four functions): kH = kW = 2, dH = dW = 2, pad 0, output_padding 0,
 *   dilation 1; any N, Cin, Cout, H, W >= 1 with N*H*W*Cin_pad, N*H*W*4*Cout_pad and N*4*H*W*Cout below 2^31 (channels padded
 *   to 64).
 *   Errors, all decided before any launch: a null tensor pointer -> TDRN_E_ARG (first); k <= 0, stride / dilation <= 0, a negative
 *   pad or output_padding, N / Cin / Cout / H / W <= 0 -> query 0 and TDRN_E_SHAPE; any other well-formed geometry -> query 0 and
 *   TDRN_E_UNSUPPORTED; a null workspace or one below the query -> TDRN_E_WORKSPACE.  One query serves all three entries.  No
 *   allocation and no host synchronisation: everything is enqueued on `stream`.
 * ====================================================================================== */
TDRN_API size_t tdrn_conv_transpose2d_workspace_bytes(int N, int Cin, int H, int W, int Cout, int kH, int kW, int dH, int dW,
                                                      int padH, int padW, int output_padH, int output_padW, int dilationH,
                                                      int dilationW, tdrn_dtype compute);
TDRN_API int tdrn_conv_transpose2d_forward(const float *input, const float *weight, const float *bias, float *output, int N,
                                           int Cin, int H, int W, int Cout, int kH, int kW, int dH, int dW, int padH, int padW,
                                           int output_padH, int output_padW, int dilationH, int dilationW, tdrn_dtype compute,
                                           void *workspace, size_t workspace_bytes, void *stream);
TDRN_API int tdrn_conv_transpose2d_backward_input(const float *grad_output, const float *weight, float *grad_input, int N,
                                                  int Cin, int H, int W, int Cout, int kH, int kW, int dH, int dW, int padH,
                                                  int padW, int output_padH, int output_padW, int dilationH, int dilationW,
                                                  tdrn_dtype compute, void *workspace, size_t workspace_bytes, void *stream);
TDRN_API int tdrn_conv_transpose2d_backward_parameters(const float *input, const float *grad_output, float *grad_weight,
                                                       float *grad_bias, int N, int Cin, int H, int W, int Cout, int kH, int kW,
                                                       int dH, int dW, int padH, int padW, int output_padH, int output_padW,
                                                       int dilationH, int dilationW, float scale, tdrn_dtype compute,
                                                       void *workspace, size_t workspace_bytes, void *stream);

/* ========================================================================================
 * (i-g) Dense 3x3 conv2d at stride 2 with gradients -- what nn.Conv2d(256, 512, 3, 2, 1) + autograd give the reference's training
 *     loop (`extras` of dualrefinedet_vggbn, ssd4scale_vgg and refinedet_vgg; nn.Conv2d(3, 32, 3, 2, 1) at the head of the MobileNet
 *     trunk): forward, input gradient, weight / bias gradient.  A family of its own: (i-c) keeps refusing stride 2, and this one
 *     refuses stride 1.
 *   Tensors, `compute`, OVERWRITTEN / += scale semantics and the argument lists are (i-c)'s, with
 *   Ho = (H + 2 pad - 3) / 2 + 1 (floor) and Wo likewise; all fp32, contiguous, device, on any 4-byte boundary.
 *   forward:             output[n][co][ho][wo] = bias[co] + sum_{ci,i,j} input[n][ci][2ho - pad + i][2wo - pad + j] weight[co][ci][i][j].
 *   backward_input:      grad_input is OVERWRITTEN: a stride-1 conv, kernel rotated and transposed, pad' = 2 - pad, over the
 *                        zero-inserted image of grad_output (H + 2 pad - 2 rows, W + 2 pad - 2 columns, grad_output[ho][wo] at
 *                        [2ho][2wo]).  An input row or column that no output pixel touches gets exactly 0.
 *   backward_parameters: grad_weight += scale * sum_p grad_output[p] input[2p - pad (+) tap], grad_bias += scale * sum_p grad_output[p],
 *                        split over K = N*Ho*Wo and summed in a fixed order.
 *   All outputs are bitwise reproducible run to run, and the same for caller buffers on any 4-byte boundary: nothing on this path
 *   uses float atomics, and the split counts depend on the geometry alone.
 *   Geometry (the argument order is the query's in all four functions): kH = kW = 3, dH = dW = 2, dilation 1,
 *   0 <= padH = padW <= 2, Ho, Wo >= 1, groups = 1.
 *   Errors, all decided before any launch: a null tensor pointer -> TDRN_E_ARG (first); k <= 0, stride / dilation <= 0, negative
 *   pad, N / Cin / Cout / H / W <= 0, an output smaller than 1 x 1 -> query 0 and TDRN_E_SHAPE; any other well-formed geometry
 *   (stride 1, per-axis stride, other kernel sizes, dilation > 1, pad > 2, per-axis pad; N*H*W*Cin_pad, N*Ho*Wo*Cout_pad or
 *   N*(H + 2 pad - 2)*(W + 2 pad - 2)*Cout_pad of 2^31 elements or more, channels padded to 64) -> query 0 and TDRN_E_UNSUPPORTED;
 *   a null workspace or one below the query -> TDRN_E_WORKSPACE.  One query serves all three entries.  No allocation and no host
 *   synchronisation: everything is enqueued on `stream`.
 * ====================================================================================== */
TDRN_API size_t tdrn_conv2d_strided_workspace_bytes(int N, int Cin, int H, int W, int Cout, int kH, int kW, int dH, int dW,
                                                    int padH, int padW, int dilationH, int dilationW, tdrn_dtype compute);
TDRN_API int tdrn_conv2d_strided_forward(const float *input, const float *weight, const float *bias, float *output, int N,
                                         int Cin, int H, int W, int Cout, int kH, int kW, int dH, int dW, int padH, int padW,
                                         int dilationH, int dilationW, tdrn_dtype compute, void *workspace,
                                         size_t workspace_bytes, void *stream);
TDRN_API int tdrn_conv2d_strided_backward_input(const float *grad_output, const float *weight, float *grad_input, int N, int Cin,
                                                int H, int W, int Cout, int kH, int kW, int dH, int dW, int padH, int padW,
                                                int dilationH, int dilationW, tdrn_dtype compute, void *workspace,
                                                size_t workspace_bytes, void *stream);
TDRN_API int tdrn_conv2d_strided_backward_parameters(const float *input, const float *grad_output, float *grad_weight,
                                                     float *grad_bias, int N, int Cin, int H, int W, int Cout, int kH, int kW,
                                                     int dH, int dW, int padH, int padW, int dilationH, int dilationW,
                                                     float scale, tdrn_dtype compute, void *workspace, size_t workspace_bytes,
                                                     void *stream);

/* ========================================================================================
 * (i-h) Depthwise 3x3 conv2d with gradients -- what nn.Conv2d(c, c, 3, s, 1, groups=c) + autograd give the reference's training loop
 *     (conv_dw, model/networks.py:736-745: the thirteen blocks of the MobileNet trunk and the two of its `extras`): forward, input
 *     gradient, weight / bias gradient, at stride 1 and 2.
 *   input (N, C, H, W), weight (C, 1, 3, 3) (torch's layout for groups = C, channel multiplier 1), bias (C) or NULL, output /
 *   grad_output (N, C, Ho, Wo) with Ho = (H + 2 pad - 3) / stride + 1 (floor) and Wo likewise, grad_input like input, grad_weight like
 *   weight, grad_bias (C) or NULL: all fp32, contiguous, device, on any 4-byte boundary.  The kernels work on the NCHW planes
 *   directly: no layout conversion, no repacked weight.
 *   forward:             output[n][c][ho][wo] = bias[c] + sum_{i,j} input[n][c][s ho - 1 + i][s wo - 1 + j] weight[c][0][i][j], nine fmaf in
 *                        the order (0,0) (0,1) .. (2,2) from the bias (or +0); a tap in the padding is skipped.  OVERWRITTEN.
 *   backward_input:      grad_input[n][c][h][w] = sum over the taps (i, j) for which h + 1 - i and w + 1 - j are multiples of the stride
 *                        with quotients inside Ho x Wo, of grad_output[n][c][(h + 1 - i) / s][(w + 1 - j) / s] weight[c][0][i][j], in
 *                        the same tap order from +0.  OVERWRITTEN; an input row or column that no output pixel touches gets exactly 0.
 *   backward_parameters: grad_weight[c][0][i][j] += scale * sum_{n,ho,wo} grad_output[n][c][ho][wo] input[n][c][s ho - 1 + i][s wo - 1 + j],
 *                        grad_bias[c] += scale * sum grad_output[.][c][.][.] (NULL: not computed).  K = N*Ho*Wo is cut into S ranges
 *                        of ceil(K / S') elements, S' = max(1, min(ceil(2048 / C), ceil(K / 1024))), S = the ranges that are not
 *                        empty; the ranges are summed in range order.
 *   `compute` must be TDRN_F32: the op is bandwidth-bound and has no 16-bit mode.
 *   forward and backward_input are that sentence bit for bit (tests/test_gpu_number_range_pointwise.py): each fmaf rounds once;
 *   subnormal inputs, products and sums are kept, never flushed; a sum past the largest finite value is +-inf.  A skipped tap is not
 *   read as 0 times its weight: a non-finite weight leaves the pixels finite for which its tap lies in the padding.  Elsewhere
 *   inf and NaN follow IEEE through the nine fmaf.  backward_parameters sums in fp32 and keeps subnormal sums as well.
 *   All outputs are bitwise reproducible run to run, and the same for caller buffers on any 4-byte boundary: nothing on this path
 *   uses float atomics, and S depends on the geometry alone.
 *   Geometry (the argument order is the query's in all four functions): kH = kW = 3, dH = dW in {1, 2}, padH = padW = 1, dilation 1;
 *   any N, C, H, W >= 1 with N*C*H*W below 2^31.
 *   The query returns 40 C S bytes rounded up to 256: the partial sums of backward_parameters.  One query serves all three entries
 *   (forward and backward_input check the workspace and do not use it).
 *   Errors, all decided before any launch, in this order: a null tensor pointer -> TDRN_E_ARG; k <= 0, stride / dilation <= 0, a
 *   negative pad, N / C / H / W <= 0, an output smaller than 1 x 1 -> query 0 and TDRN_E_SHAPE; `compute` outside 0..2 -> TDRN_E_ARG;
 *   any other well-formed geometry (other kernel sizes, stride 3, per-axis stride or pad, pad 0 or 2, dilation 2, TDRN_BF16 /
 *   TDRN_F16, N*C*H*W of 2^31 or more) -> query 0 and TDRN_E_UNSUPPORTED; a null workspace or one below the query ->
 *   TDRN_E_WORKSPACE.  No allocation and no host synchronisation: everything is enqueued on `stream`.
 * ====================================================================================== */
TDRN_API size_t tdrn_dwconv2d_workspace_bytes(int N, int C, int H, int W, int kH, int kW, int dH, int dW, int padH, int padW,
                                              int dilationH, int dilationW, tdrn_dtype compute);
TDRN_API int tdrn_dwconv2d_forward(const float *input, const float *weight, const float *bias, float *output, int N, int C, int H,
                                   int W, int kH, int kW, int dH, int dW, int padH, int padW, int dilationH, int dilationW,
                                   tdrn_dtype compute, void *workspace, size_t workspace_bytes, void *stream);
TDRN_API int tdrn_dwconv2d_backward_input(const float *grad_output, const float *weight, float *grad_input, int N, int C, int H,
                                          int W, int kH, int kW, int dH, int dW, int padH, int padW, int dilationH, int dilationW,
                                          tdrn_dtype compute, void *workspace, size_t workspace_bytes, void *stream);
TDRN_API int tdrn_dwconv2d_backward_parameters(const float *input, const float *grad_output, float *grad_weight, float *grad_bias,
                                               int N, int C, int H, int W, int kH, int kW, int dH, int dW, int padH, int padW,
                                               int dilationH, int dilationW, float scale, tdrn_dtype compute, void *workspace,
                                               size_t workspace_bytes, void *stream);

/* ========================================================================================
 * (i-i) Dense 5x5 conv2d with gradients -- what nn.Conv2d(256, c, 5, 1, 2) + autograd give the reference's training loop (odm_loc_2 /
 *     odm_conf_2 of refinedet_vgg with multihead=True): forward, input gradient, weight / bias gradient.  A family of its own: (i-c)
 *     keeps refusing k = 5, and this one refuses every other kernel size.
 *   Tensors, `compute`, OVERWRITTEN / += scale semantics, the argument lists and the order of the checks are (i-c)'s, with
 *   Ho = H and Wo = W; all fp32, contiguous, device, on any 4-byte boundary.
 *   forward:             output[n][co][h][w] = bias[co] + sum_{ci,i,j} input[n][ci][h - 2 + i][w - 2 + j] weight[co][ci][i][j].
 *   backward_input:      grad_input is OVERWRITTEN: the same conv over grad_output with the kernel rotated by 180 degrees and its
 *                        channel axes exchanged (pad' = 4 - 2 = 2).
 *   backward_parameters: grad_weight += scale * sum_p grad_output[p] input[p - 2 (+) tap], grad_bias += scale * sum_p grad_output[p]
 *                        (NULL: not computed), split over K = N*H*W and summed in split order.  The 25 taps run as five passes, one
 *                        per kernel row, side by side in one launch; K is cut into S = ceil(K / P) ranges of
 *                        P = ceil(ceil(K / S') / 64) * 64 pixels, S' = max(1, min(ceil(512 / (5 T)), ceil(K / 256))), T = the 64 x 64
 *                        tiles of the padded Cout x Cin.
 *   All outputs are bitwise reproducible run to run, and the same for caller buffers on any 4-byte boundary: nothing on this path
 *   uses float atomics, and the split counts depend on the geometry alone.
 *   Geometry (the argument order is the query's in all four functions): kH = kW = 5, dH = dW = 1, dilation 1, padH = padW = 2,
 *   groups = 1; any N, Cin, Cout, H, W >= 1 inside the limits below.
 *   Errors, all decided before any launch: a null tensor pointer -> TDRN_E_ARG (first); k <= 0, stride / dilation <= 0, negative
 *   pad, N / Cin / Cout / H / W <= 0, an output smaller than 1 x 1 -> query 0 and TDRN_E_SHAPE; `compute` outside 0..2 -> TDRN_E_ARG;
 *   any other well-formed geometry (k = 1 or 3 or any other size, a non-square kernel, stride 2, pad 1 or 3, per-axis pad, dilation 2;
 *   N*H*W*Cin_pad or N*H*W*Cout_pad of 2^31 elements or more, channels padded to 64) -> query 0 and TDRN_E_UNSUPPORTED; a null
 *   workspace or one below the query -> TDRN_E_WORKSPACE.  One query serves all three entries.  No allocation and no host
 *   synchronisation: everything is enqueued on `stream`.
 * ====================================================================================== */
TDRN_API size_t tdrn_conv5x5_workspace_bytes(int N, int Cin, int H, int W, int Cout, int kH, int kW, int dH, int dW, int padH,
                                             int padW, int dilationH, int dilationW, tdrn_dtype compute);
TDRN_API int tdrn_conv5x5_forward(const float *input, const float *weight, const float *bias, float *output, int N, int Cin,
                                  int H, int W, int Cout, int kH, int kW, int dH, int dW, int padH, int padW, int dilationH,
                                  int dilationW, tdrn_dtype compute, void *workspace, size_t workspace_bytes, void *stream);
TDRN_API int tdrn_conv5x5_backward_input(const float *grad_output, const float *weight, float *grad_input, int N, int Cin,
                                         int H, int W, int Cout, int kH, int kW, int dH, int dW, int padH, int padW,
                                         int dilationH, int dilationW, tdrn_dtype compute, void *workspace,
                                         size_t workspace_bytes, void *stream);
TDRN_API int tdrn_conv5x5_backward_parameters(const float *input, const float *grad_output, float *grad_weight,
                                              float *grad_bias, int N, int Cin, int H, int W, int Cout, int kH, int kW, int dH,
                                              int dW, int padH, int padW, int dilationH, int dilationW, float scale,
                                              tdrn_dtype compute, void *workspace, size_t workspace_bytes, void *stream);

/* ========================================================================================
 * (i-j) SGD, one fused step over a list of fp32 tensors -- what optimizer.step() of optim.SGD(net.parameters(), lr, momentum,
 *     weight_decay) gives the reference's training loops (train.py:259-270, train_trn.py:218-221), with the learning rate read on
 *     the device (adjust_learning_rate, train.py:321-328, changes it every iteration during warm-up).
 *   tensors_host (n_tensors) HOST records {param, grad, momentum_buf: DEVICE fp32, contiguous, numel elements each, on any 4-byte
 *   boundary; group}; the records are copied into kernel arguments before the call returns.  hyper_dev (n_groups, 4) DEVICE fp32
 *   rows {lr, momentum, weight_decay, nesterov as 0 / 1}, read by the kernel when it runs: a captured step replayed after the row
 *   was rewritten uses the new values.  Per element, with (lr, mom, wd, nesterov) the row of the tensor's group, every operation
 *   rounded to fp32 on its own (nothing is contracted into an fma):
 *       d = (wd != 0) ? g + wd*p : g
 *       if (mom != 0) { b = mom*b + d;  u = nesterov ? d + mom*b : b; } else u = d
 *       p = p - lr*u
 *       if (flags & TDRN_SGD_ZERO_GRADS) g = +0
 *   momentum_buf starts as zeros (the caller's job), so the first step is no special case and a captured step is the same in every
 *   replay.  torch.optim.SGD starts with buf = clone(d) instead; b = mom*0 + d equals that except for the sign of a zero: where
 *   d = -0 the buffer holds +0.  momentum_buf is neither read nor written when mom == 0, but must be a valid pointer all the same
 *   (the host cannot read hyper_dev).  Dampening and maximize are not covered.
 *   The five lines hold over the whole of fp32 (tests/test_gpu_number_range_pointwise.py): subnormal p, g, b, lr and products are
 *   read and kept as what they are (lr*u below 2^-150 is +-0, nothing is flushed earlier), the sign of a zero follows IEEE, lr*u past
 *   the largest finite value is +-inf, and inf / NaN in g reach p and b of that element by IEEE's rules and no other element.
 *   A record with numel = 0 or a null grad is skipped (torch skips grad is None the same way); nothing else of it is looked at but
 *   numel and group.  The other records go out in launches of up to TDRN_SGD_TENSORS_PER_LAUNCH tensors each, in chunks of
 *   TDRN_SGD_CHUNK elements, with 16-byte vector accesses where param, grad and momentum_buf are all 16-byte aligned and scalar
 *   ones elsewhere (the numel % 4 tail is always scalar).
 *   All outputs are bitwise reproducible run to run and for caller buffers on any 4-byte boundary: no atomics, and each element's
 *   result depends on that element alone.
 *   Errors, all decided before any launch: a null tensors_host or hyper_dev, n_tensors < 0, n_groups < 1, unknown flag bits, and per
 *   record a negative numel, a group outside [0, n_groups), and (unless skipped) a null param or momentum_buf -> TDRN_E_ARG; a
 *   numel of 2^31 or more -> TDRN_E_UNSUPPORTED.  No workspace, no allocation and no host synchronisation: everything is enqueued
 *   on `stream`.
 * ====================================================================================== */
#define TDRN_SGD_ZERO_GRADS 1
#define TDRN_SGD_CHUNK 4096              /* elements a workgroup handles at a time */
#define TDRN_SGD_TENSORS_PER_LAUNCH 96   /* descriptors one launch carries in its arguments */
typedef struct {
    float *param;
    float *grad;             /* NULL: the tensor is skipped */
    float *momentum_buf;
    int64_t numel;
    int32_t group;           /* row of hyper_dev */
    int32_t reserved;
} tdrn_sgd_tensor;
TDRN_API int tdrn_sgd_step(const tdrn_sgd_tensor *tensors_host, int n_tensors, const float *hyper_dev, int n_groups, int flags,
                           void *stream);

/* ========================================================================================
 * (i-k) Resident training tensors: conv2d, BatchNorm2d (+ ReLU) and MaxPool2d whose activations and activation gradients stay in
 *     16-bit NHWC between layers, so that a layer converts no layout and the convs may run on the inference engine's 3x3 kernels.
 *   A RESIDENT TENSOR of logical shape (N, C, H, W) is `dtype` = TDRN_BF16 or TDRN_F16 memory [N][H][W][C] without gaps (torch:
 *   contiguous in channels_last), C % 64 == 0, on a 16-byte boundary, fewer than 2^31 elements.  Activations and their gradients
 *   are resident tensors of the same type; parameters, their gradients, the BatchNorm buffers and all statistics stay fp32 as in
 *   (i-c) .. (i-e).  All accumulation is fp32; a conv output and a BatchNorm output are each rounded ONCE to the type, to nearest
 *   even: a result in the type's subnormal range is kept at the subnormal spacing (never flushed), one past the largest finite value
 *   becomes +-inf (65504 + 16 in fp16; nothing saturates), and subnormal activations are read as what they are
 *   (tests/test_gpu_number_range_resident.py, on every route of the conv); at the layout boundary NaN stays NaN as well (NaN and
 *   +-inf through the conv and BatchNorm epilogues are not measured).  Argument lists mirror the fp32 NCHW entries they stand beside.  Nothing allocates, nothing synchronises, everything is
 *   enqueued on `stream`; no float atomics, every output is bitwise reproducible.
 *   Errors, all decided before any launch, in this order per entry: a null pointer, an activation pointer off a 16-byte boundary, an
 *   fp32 pointer off a 4-byte one, a dtype other than TDRN_BF16 / TDRN_F16 (TDRN_F32 included), unknown flag bits -> TDRN_E_ARG; the
 *   shape checks of the fp32 entry -> TDRN_E_SHAPE; geometry outside the fp32 entry's family, a channel count C (Cin, Cout) with
 *   C % 64 != 0, 2^31 or more elements -> TDRN_E_UNSUPPORTED; a null or short workspace -> TDRN_E_WORKSPACE.
 *
 *   Layout boundary.  tdrn_nhwc16_from_nchw: fp32 NCHW (N, C, H, W) -> resident, each value rounded once; tdrn_nchw_from_nhwc16 the
 *   way back (exact).  Each is the other's backward.
 *
 *   tdrn_conv2d_nhwc_*: the geometry of (i-c) (square k = 1 | 3, stride 1, one pad / dilation, pad <= dilation (k - 1)) with
 *   Cin % 64 == 0 and Cout % 64 == 0.  weight (OIHW) and bias are fp32 and rounded once when they are packed; bias is not rounded.
 *   forward reads `input` and writes `output` in place -- no conversion kernel, no copy of the result; backward_input is the same
 *   launch over grad_output with the rotated, transposed kernel and pad' = dilation (k - 1) - pad, and writes grad_input directly;
 *   backward_parameters is the (i-c) weight-gradient GEMM straight on the two caller tensors: grad_weight / grad_bias (fp32) +=
 *   scale * their sums.  Workspace: zero page | packed weight | padded bias | split-K partials or the weight gradient's slabs.  No
 *   launch of these entries polls a flag written by another workgroup.  `flags`: TDRN_CONV_NHWC_IGEMM_ONLY keeps forward and
 *   backward_input on the generic implicit GEMM (conv_igemm.hip) instead of the 3x3 direct-conv kernels and the wide 1x1 GEMM, for
 *   comparison.  The split-K choice stays that of the default route (so the workspace size does not change; the query takes the
 *   flag all the same), but the two routes do NOT sum in the same fp32 order: the direct-conv kernels start their accumulators at the
 *   bias and step through (64-channel chunk, tap), conv_igemm.hip steps through (tap, chunk) and adds the bias last.  The results
 *   are bit-equal only for a launch that convolves ONE 64-channel chunk and has no (or a zero) bias -- forward: Cin = 64, bias NULL;
 *   backward_input: Cout = 64 --; otherwise they agree up to the one rounding of the result (a few elements per ten thousand differ
 *   in the last places).  tdrn_conv2d_nhwc_route names the kernel forward (dgrad = 0) or backward_input (dgrad = 1) reaches
 *   ("igemm", "patch", "pp", "pw1x1"), NULL where the entries refuse; tdrn_conv2d_nhwc_splits gives the K slices of launch_conv's
 *   split-K in the forward and in backward_input (1 = none) and the K splits of the weight gradient; both make no GPU call.
 *
 *   tdrn_batch_norm_nhwc_*: (i-d)'s semantics -- training / eval, momentum, eps, relu, fp32 save_mean / save_invstd, the running
 *   buffers moved once, NULL grad_input or NULL (grad_weight, grad_bias) dropping the kernels that compute them -- with input,
 *   output, grad_output and grad_input resident.  z = fma(x - mean, gamma invstd, beta) in fp32, the ReLU acts on z before the one
 *   rounding, and the backward recomputes the mask z > 0 from `input`.  A workgroup owns 64 channels and one of `splits` ranges of
 *   per_split pixel rows: S = clamp(floor(2048 / (C / 64)), 1, ceil(M / 256)), M = N H W, per_split = ceil(M / S) rounded up to 32,
 *   splits = ceil(M / per_split) (tdrn_batch_norm_nhwc_splits: a pure function of the shape; returns a status).  Statistics are
 *   (count, mean, M2) records merged by Chan's formula in a fixed order, the splits in float64.  Workspace: 12 C splits + 8 C bytes.
 *   The records and their merge are (i-d)'s (bn_prims.h), and so is the range of the statistics: right at any scale and any mean
 *   while M (max x - min x)^2 < 2^128, M2 = +inf -> save_invstd = 0 -> output = bias past it.  Every finite fp16 input is inside the
 *   range (65504^2 M < 2^128); bf16 inputs past 2^63 can leave it.
 *
 *   tdrn_max_pool_nhwc_*: (i-e)'s three geometries, selection rule and one-byte codes, the codes laid out like the output
 *   ([N][Ho][Wo][C], on any byte; NULL in the forward: none are written).  backward reads grad_output and codes only and writes
 *   every element of grad_input once; 3x3 sums in window row-major order in fp32 from +0.0 and rounds once.
 * ====================================================================================== */
#define TDRN_CONV_NHWC_IGEMM_ONLY 1
TDRN_API int tdrn_nhwc16_from_nchw(const float *in, void *out, int N, int C, int H, int W, tdrn_dtype dtype, void *stream);
TDRN_API int tdrn_nchw_from_nhwc16(const void *in, float *out, int N, int C, int H, int W, tdrn_dtype dtype, void *stream);
TDRN_API size_t tdrn_conv2d_nhwc_workspace_bytes(int N, int Cin, int H, int W, int Cout, int kH, int kW, int dH, int dW, int padH,
                                                 int padW, int dilationH, int dilationW, tdrn_dtype dtype, int flags);
TDRN_API int tdrn_conv2d_nhwc_forward(const void *input, const float *weight, const float *bias, void *output, int N, int Cin, int H,
                                      int W, int Cout, int kH, int kW, int dH, int dW, int padH, int padW, int dilationH, int dilationW,
                                      tdrn_dtype dtype, void *workspace, size_t workspace_bytes, void *stream, int flags);
TDRN_API int tdrn_conv2d_nhwc_backward_input(const void *grad_output, const float *weight, void *grad_input, int N, int Cin, int H,
                                             int W, int Cout, int kH, int kW, int dH, int dW, int padH, int padW, int dilationH,
                                             int dilationW, tdrn_dtype dtype, void *workspace, size_t workspace_bytes, void *stream,
                                             int flags);
TDRN_API int tdrn_conv2d_nhwc_backward_parameters(const void *input, const void *grad_output, float *grad_weight, float *grad_bias,
                                                  int N, int Cin, int H, int W, int Cout, int kH, int kW, int dH, int dW, int padH,
                                                  int padW, int dilationH, int dilationW, float scale, tdrn_dtype dtype,
                                                  void *workspace, size_t workspace_bytes, void *stream, int flags);
TDRN_API const char *tdrn_conv2d_nhwc_route(int N, int Cin, int H, int W, int Cout, int kH, int kW, int dH, int dW, int padH, int padW,
                                            int dilationH, int dilationW, tdrn_dtype dtype, int flags, int dgrad);
TDRN_API int tdrn_conv2d_nhwc_splits(int N, int Cin, int H, int W, int Cout, int kH, int kW, int dH, int dW, int padH, int padW,
                                     int dilationH, int dilationW, tdrn_dtype dtype, int flags, int *splitk_forward, int *splitk_dgrad,
                                     int *wgrad_splits);
TDRN_API int tdrn_batch_norm_nhwc_splits(int N, int C, int H, int W, int *splits, int *per_split);
TDRN_API size_t tdrn_batch_norm_nhwc_workspace_bytes(int N, int C, int H, int W);
TDRN_API int tdrn_batch_norm_nhwc_forward(const void *input, const float *weight, const float *bias, float *running_mean,
                                          float *running_var, void *output, float *save_mean, float *save_invstd, int N, int C, int H,
                                          int W, int training, float momentum, float eps, int relu, tdrn_dtype dtype, void *workspace,
                                          size_t workspace_bytes, void *stream);
TDRN_API int tdrn_batch_norm_nhwc_backward(const void *input, const void *grad_output, const float *weight, const float *bias,
                                           const float *save_mean, const float *save_invstd, void *grad_input, float *grad_weight,
                                           float *grad_bias, int N, int C, int H, int W, int training, int relu, float scale,
                                           tdrn_dtype dtype, void *workspace, size_t workspace_bytes, void *stream);
TDRN_API int tdrn_max_pool_nhwc_forward(const void *input, void *output, unsigned char *code, int N, int C, int H, int W, int kernel,
                                        int stride, int pad, int ceil_mode, tdrn_dtype dtype, void *stream);
TDRN_API int tdrn_max_pool_nhwc_backward(const void *grad_output, const unsigned char *code, void *grad_input, int N, int C, int H,
                                         int W, int kernel, int stride, int pad, int ceil_mode, tdrn_dtype dtype, void *stream);

/* ========================================================================================
 * (i-l) Deformable convolution v1 with gradients in the transform domain ("transform, then sample") -- an opt-in second algorithm
 *     beside (i) / (i-b), for one deformable group and a 16-bit compute type.  A deformable conv is linear in the sampled values:
 *     with b(p,t,q) the bilinear coefficient of input pixel q for the sample of output pixel p at tap t (the sampling rule of (i):
 *     rejection outside the map, the [H-1, H) clamp band, fp32 coordinates),
 *         Y_t[n,co,q]      = sum_c W[co,c,t] X[n,c,q]                   1x1 GEMM on un-deformed pixels (MFMA)
 *         out[n,co,p]      = sum_t sum_q b(p,t,q) Y_t[n,co,q]           sampling, Cout wide
 *         Z_t[n,co,q]      = sum_p b(p,t,q) gO[n,co,p]                  scatter, Cout wide (fp32 atomics)
 *         grad_input       = sum_t sum_co W[co,c,t] Z_t[n,co,q]         1x1 GEMM, K = kH kW Cout (MFMA)
 *         grad_weight      = sum_{n,q} Z_t[n,co,q] X[n,c,q]             1x1 weight-gradient GEMM, K = N H W (MFMA)
 *         grad_offset[p,t] = sum_co gO[n,co,p] d/dpos sum_q b(p,t,q) Y_t[n,co,q]
 *   Tensors and the order of the geometry arguments are (i)'s: input, offset, output, grad_output, the three gradients fp32 NCHW,
 *   weight OIHW fp32; every fp32 pointer on a 4-byte boundary.  Y is (N, H, W, YC) in `dtype`, YC = kH kW ceil8(Cout) rounded up to a
 *   multiple of 64, tdrn_deform_conv_ts_y_bytes bytes on a 16-byte boundary.
 *   Scope: deformable_group = 1; dtype TDRN_BF16 or TDRN_F16; Cin % 64 == 0; 1 <= Cout <= 256; any kernel, stride, padding and
 *   dilation (i-b) accepts (Y lives on input pixels, so Ho x Wo need not be H x W).  Outside it: TDRN_E_UNSUPPORTED; so is any
 *   buffer (a tensor, Y, Z) of 2^31 elements or more.  A NULL or misaligned required pointer: TDRN_E_ARG; a failed shape_check:
 *   TDRN_E_SHAPE; a short workspace: TDRN_E_WORKSPACE.  Every refusal is decided before the first launch.  The queries are pure
 *   host functions and return 0 where the entries refuse.  No allocation, no host synchronisation: everything is enqueued on `stream`.
 *   Numerics: X, W and Z are rounded ONCE to `dtype`, to nearest even; Y is the GEMM's fp32 sum rounded once; everything else is
 *   fp32 (the four bilinear weights are the reference's fp32 products; taps are summed in tap order).
 *   forward:  output is OVERWRITTEN.  y_save: NULL, or it receives Y for the backward.
 *   backward: ONE entry, so that Z is scattered once and serves grad_input and grad_weight.  Each of grad_input, grad_offset and
 *     grad_weight may be NULL (not all three) and is OVERWRITTEN otherwise; work that nobody asked for is skipped: grad_offset needs
 *     no Z, grad_input and grad_weight need no Y.  y_saved: the forward's Y, or NULL: Y is recomputed (the same bits).  grad_offset
 *     has the one-sided derivative at integer coordinates and a zero derivative along an axis inside its clamp band, as (i-b).
 *   Reproducibility: output, Y and grad_offset are bitwise reproducible (no atomics, fixed summation orders).  grad_input and
 *     grad_weight are not: the float atomics into Z arrive in any order, as with (i-b)'s grad_input; behind Z every sum has a
 *     fixed order.
 * ====================================================================================== */
TDRN_API size_t tdrn_deform_conv_ts_workspace_bytes(int N, int Cin, int H, int W, int Cout, int kW, int kH, int dW, int dH, int padW,
                                                    int padH, int dilationH, int dilationW, int deformable_group, tdrn_dtype dtype);
TDRN_API size_t tdrn_deform_conv_ts_y_bytes(int N, int Cin, int H, int W, int Cout, int kW, int kH, int dW, int dH, int padW, int padH,
                                            int dilationH, int dilationW, int deformable_group, tdrn_dtype dtype);
TDRN_API int tdrn_deform_conv_ts_forward(const float *input, const float *weight, const float *offset, float *output, void *y_save,
                                         int N, int Cin, int H, int W, int Cout, int kW, int kH, int dW, int dH, int padW, int padH,
                                         int dilationH, int dilationW, int deformable_group, tdrn_dtype dtype, void *workspace,
                                         size_t workspace_bytes, void *stream);
TDRN_API int tdrn_deform_conv_ts_backward(const float *input, const float *weight, const float *offset, const float *grad_output,
                                          const void *y_saved, float *grad_input, float *grad_offset, float *grad_weight, int N,
                                          int Cin, int H, int W, int Cout, int kW, int kH, int dW, int dH, int padW, int padH,
                                          int dilationH, int dilationW, int deformable_group, tdrn_dtype dtype, void *workspace,
                                          size_t workspace_bytes, void *stream);

/* ========================================================================================
 * (i-m) Dynamic loss scaling for fp16 training -- what torch.cuda.amp.GradScaler gives a CUDA user, with every decision taken on
 *     the device: the loss is multiplied by a scale so that fp16 activation gradients stay above the type's smallest subnormal,
 *     the SGD step of (i-j) divides the scale out again, and a step whose gradients hold inf or NaN is skipped and halves the scale.
 *   state_dev: four DEVICE fp32 words on a 16-byte boundary, {scale, good_steps, found_inf, skipped}.  The two counts are held as
 *   floats and are exact below 2^24; found_inf is 0 or 1.  The kernels read and write them when they run: a captured step replayed
 *   after the scale moved uses the new scale.  tensors_host, hyper_dev, n_groups and flags are (i-j)'s.
 *   tdrn_amp_check_finite: reads every gradient element of the records that (i-j) would not skip (16-byte vector loads where grad is
 *   16-byte aligned, scalar ones elsewhere and in the numel % 4 tail) and, if one is +-inf or NaN, stores found_inf = 1.  It never
 *   stores 0: the flag stays up over any number of checks until tdrn_amp_update, so two optimizers may share one state.  The
 *   largest finite value and subnormals are finite.  param and momentum_buf are not looked at and may be null.
 *   tdrn_sgd_step_scaled: (i-j)'s step with, read from state_dev when it runs,
 *       inv = 1 / scale                       one fp32 division
 *       g'  = g * inv                         one fp32 rounding; g' takes g's place in the four lines of (i-j)
 *       if (found_inf != 0) no element of param or momentum_buf of any tensor of any launch of the call is written
 *       if (flags & TDRN_SGD_ZERO_GRADS) g = +0, skipped or not
 *   It writes nothing to state_dev.  With scale = 1 and found_inf = 0 its results are tdrn_sgd_step's bit for bit.  The check is
 *   a call of its own because a list may go out in several launches: a non-finite gradient in the last launch must stop the first.
 *   tdrn_amp_update: torch's _amp_update_scale_, in fp32, by one lane:
 *       if (found_inf != 0) { scale = scale * backoff_factor;  good_steps = 0;  skipped += 1; }
 *       else { good_steps += 1;
 *              if (good_steps == growth_interval) { s = scale * growth_factor;  if (isfinite(s)) scale = s;  good_steps = 0; } }
 *       found_inf = 0
 *   (torch multiplies by the factor as a double; with factors that fp32 holds exactly the two agree bit for bit.)
 *   All results are bitwise reproducible run to run: no atomics; every writer of found_inf stores the same word.
 *   Errors, all decided before any launch, in (i-j)'s order: a null tensors_host or hyper_dev, n_tensors < 0, n_groups < 1, a null
 *   state_dev or one off a 16-byte boundary, unknown flag bits, growth_factor <= 1, backoff_factor outside the open interval (0, 1),
 *   growth_interval < 1 or >= 1 << 24, and the record errors of (i-j) -> TDRN_E_ARG (tdrn_amp_check_finite has no rows to hold a
 *   group against: it rejects a negative group, and requires neither param nor momentum_buf); a numel of 2^31 or more ->
 *   TDRN_E_UNSUPPORTED.  No workspace, no allocation and no host synchronisation: everything is enqueued on `stream`, and all three
 *   entries are legal under stream capture.
 * ====================================================================================== */
TDRN_API int tdrn_amp_check_finite(const tdrn_sgd_tensor *tensors_host, int n_tensors, float *state_dev, void *stream);
TDRN_API int tdrn_sgd_step_scaled(const tdrn_sgd_tensor *tensors_host, int n_tensors, const float *hyper_dev, int n_groups,
                                  const float *state_dev, int flags, void *stream);
TDRN_API int tdrn_amp_update(float *state_dev, float growth_factor, float backoff_factor, int growth_interval, void *stream);

/* ========================================================================================
 * (ii) NMS / box utilities / Detect
 * ====================================================================================== */

/* Greedy NMS with the CPU semantics Detect uses -- replaces
 *     cpu_nms(ndarray[float32, ndim=2] dets, float thresh) -> list   utils/nms/cpu_nms.pyx:17-68
 *     (dispatcher utils/nms_wrapper.py:23-31, called at layers/functions/detection.py:60)
 *   dets (n,5) device fp32 rows [x1,y1,x2,y2,score] in pixel units ("+1" convention), ANY order;
 *   any n (above 16384 boxes the sort keys live in the workspace instead of LDS);
 *   sorted on device by (score desc, index asc).  Suppression when IoU >= thresh
 *   (strict_gt = 0, cpu_nms.pyx:66) or IoU > thresh (strict_gt = 1, nms_kernel.cu:71); the IoU
 *   is fp32 and compared against the double `thresh` exactly as the Cython code does.
 *   keep_out (n) device int32 <- kept indices into dets, descending score; num_out (1) device. */
TDRN_API size_t tdrn_nms_workspace_bytes(int n);
TDRN_API int tdrn_nms(const float *dets, int n, double thresh, int strict_gt, int32_t *keep_out,
                      int32_t *num_out, void *workspace, size_t workspace_bytes, void *stream);

/* The torch NMS that DetectOTA uses -- replaces
 *     nms(boxes, scores, overlap=0.5, top_k=200) -> (keep, count)       layers/box_utils.py:229-293
 *   dets (n,5) device fp32 rows [x1,y1,x2,y2,score], normalised coordinates, NO "+1": area = (x2-x1)*(y2-y1),
 *   IoU = inter / ((area_j - inter) + area_i) in fp32; a candidate survives iff IoU <= overlap (fp32).  Only boxes
 *   with score > min_score are candidates (the caller's c_mask, detection_ota.py:67-68) and only the top_k best
 *   of them enter (box_utils.py:251; 0 = all).  keep_out (n) <- kept indices into dets, descending score. */
TDRN_API int tdrn_nms_topk(const float *dets, int n, float overlap, float min_score, int top_k,
                           int32_t *keep_out, int32_t *num_out, void *workspace,
                           size_t workspace_bytes, void *stream);

/* The per-class loop of DetectOTA.forward (layers/functions/detection_ota.py:61-79: for cl in 1..C-1: c_mask, nms(boxes,
 * scores, nms_thresh, top_k)) as ONE launch: boxes (n,4) shared by all classes, scores (n, num_classes) row-major (the softmax
 * output of one frame); class c in [first_class, num_classes) runs tdrn_nms_topk's rule on (boxes, scores[:, c]).
 * keep_out (num_classes, n) int32 and num_out (num_classes): rows below first_class are not written.  n <= 16384
 * (TDRN_E_UNSUPPORTED beyond: call tdrn_nms_topk per class).  No host round trip: the caller reads num_out once. */
TDRN_API size_t tdrn_nms_topk_classes_workspace_bytes(int n, int num_classes);
TDRN_API int tdrn_nms_topk_classes(const float *boxes, const float *scores, int n, int num_classes, int first_class,
                                   float overlap, float min_score, int top_k, int32_t *keep_out, int32_t *num_out,
                                   void *workspace, size_t workspace_bytes, void *stream);

/* DetectOTA's association arithmetic on the device (the reference does it with torch ops on the GPU; here it is two kernels).
 * tdrn_roi_resample -- detection_ota.py:86-93: for box b the cell range [x0,x1) x [y0,y1) of the (C,H,W) fp32 feature map
 *   (cells (n,4) int32 = x0,y0,x1,y1, computed by the caller as the reference does: floor / ceil of box * size, clipped) is resampled
 *   to S x S with F.upsample(mode='bilinear', align_corners=True)'s arithmetic and flattened as (C,S,S): out (n, C*S*S) fp32.
 * tdrn_ota_similarity -- detection_ota.py:95-99 with box_utils.IoU / cos_similarity (layers/box_utils.py:295-367):
 *   sim[i][j] = exp(IoU(boxes[i], head_j)) * mean_r cos(roi[i], feature of row r of tubelet j); best[i] = max_j, arg[i] = its index.
 *   rows (R, 5+F) fp32: the stored rows [score, x1,y1,x2,y2, feature] of all m tubelets back to back, a tubelet's newest row (its
 *   head) first; row_off (m+1) int32: tubelet j = rows [row_off[j], row_off[j+1]).  No host round trip. */
TDRN_API int tdrn_roi_resample(const float *feature, int C, int H, int W, const int32_t *cells, int n, int S, float *out,
                               void *stream);
TDRN_API int tdrn_ota_similarity(const float *boxes, const float *roi, int n, int F, const float *rows, const int32_t *row_off,
                                 int m, float *best, int32_t *arg, void *stream);

/* COMPAT twin of   void _nms(int* keep_out, int* num_out, const float* boxes_host,
 *     int boxes_num, int boxes_dim, float nms_overlap_thresh, int device_id)
 *                                                          utils/nms/gpu_nms.hpp:1-2
 *   HOST pointers in and out, boxes already sorted descending by the caller
 *   (gpu_nms.pyx:25-28), strict `>` threshold (nms_kernel.cu:71), synchronous, allocates and
 *   frees device memory per call like the reference (nms_kernel.cu:100-143).  Not hot path. */
TDRN_API int tdrn_gpu_nms_host(int *keep_out, int *num_out, const float *boxes_host,
                               int boxes_num, int boxes_dim, float nms_overlap_thresh,
                               int device_id);

/* decode / center_size -- layers/box_utils.py:176-195, :16-25.  Device fp32 (P,4) arrays, each 16-byte aligned (the rows are
 * read and written as 16-byte vectors): any other address -> TDRN_E_ARG, checked on the host before anything is enqueued. */
TDRN_API int tdrn_decode(const float *loc, const float *priors, int P, float var0, float var1,
                         float *boxes_out, void *stream);
TDRN_API int tdrn_center_size(const float *boxes, int P, float *out, void *stream);

/* ========================================================================================
 * (ii-b) Training losses, fp32 -- replace
 *     match(threshold, truths, priors, variances, labels, loc_t, conf_t, idx)     layers/box_utils.py:81-121
 *     refine_match(..., idx, arm_loc)                                              :123-149
 *     MultiBoxLoss.forward / RefineMultiBoxLoss.forward      layers/modules/multibox_loss.py:59-110,
 *                                                            layers/modules/refine_multibox_loss.py:28-102
 *   and their autograd backward.  Semantics are the reference's, quirks included:
 *   - IoU: truths against point_form(priors) (match) or against the ARM decode of the priors (refine_match; the decode is
 *     tdrn_decode's arithmetic); op order of intersect / jaccard (:28-67): inter = clamp(min(x2)-max(x1),0) *
 *     clamp(min(y2)-max(y1),0), union = (area_a + area_b) - inter, iou = inter / union, correctly rounded.
 *   - argmax ties go to the lowest index (torch CPU): a prior that overlaps no truth takes truth 0, a truth that overlaps
 *     no prior takes prior 0.  Forced matches: overlap 2 at every truth's best prior, then in ascending j
 *     best_truth_idx[best_prior_idx[j]] = j, so when truths share a best prior the LAST j wins.
 *   - conf_t = (int)(label + 1) (the float -> long truncation), 0 where the overlap is below `threshold`.
 *   - encode (:151-172) op for op, against the priors (match) or center_size(decoded) (refine_match).
 *   - an image with no truths: all background, loc_t = 0, no positives and so no mined negatives (the reference fails).
 *   - mining score: log_sum_exp with the BATCH-global max of conf (box_utils.py:216-223) minus the target logit; rows whose
 *     exps all underflow score -inf and rank last; positives score 0.  num_neg = min(negpos_ratio * num_pos, P - 1) per
 *     image; a row is a negative when its rank in a STABLE descending sort of the score is below num_neg (ties: the lower
 *     prior index first).  A positive that ranks in is counted once (pos u neg).
 *   - loss_l = smooth-L1 (beta 1, summed) over positives; loss_c = cross entropy (summed, per-row log-softmax) over
 *     pos u neg; both divided by N = sum of num_pos as float.  N = 0 gives 0/0 = NaN, as the reference's arithmetic.
 *   - backward: d/d loc = g_l / N * clamp(loc - loc_t, -1, 1) on positives, d/d conf = g_c / N * (softmax(conf) -
 *     onehot(conf_t)) on pos u neg, 0 elsewhere; targets and arm_loc get no gradient (the reference detaches them).
 *   prior_for_matching, bkg_label, neg_mining, neg_overlap, encode_target are unused by the reference and have no argument.
 *
 * tdrn_match: B images in one call.  truths (T_total, 5) device fp32 rows [x1,y1,x2,y2,label], image b = rows
 *   [truth_off[b], truth_off[b+1]) with truth_off (B+1) int32 DEVICE; every image has at most max_truths rows (<= 512,
 *   else TDRN_E_UNSUPPORTED; offsets that break the promise are clamped, never followed out of bounds).  truths may be
 *   NULL when T_total = 0.  priors (P,4) center-size; arm_loc (B,P,4) or NULL (NULL: match, else refine_match).
 *   loc_t (B,P,4) fp32 and conf_t (B,P) int32, fully overwritten.
 * tdrn_multibox_loss_forward: loc (B,P,4), conf (B,P,C) or NULL (= only_loc: no mining, loss_out[1] untouched), loc_t,
 *   conf_t as tdrn_match writes them.  C <= 1024 (TDRN_E_UNSUPPORTED above).  Outputs, all device: loss_out (2) fp32 =
 *   [loss_l / N, loss_c / N]; sel (B,P) uint8 = 0 unused, 1 positive, 2 mined negative; num_pos (B) int32.
 *   The workspace query takes C = 0 for only_loc.
 * tdrn_multibox_loss_backward: grad_loss (2) DEVICE fp32 = [d/d loss_l, d/d loss_c] (read on the device: no host round
 *   trip); sel and num_pos of the forward; grad_loc (B,P,4) and grad_conf (B,P,C) fully overwritten (grad_conf unused
 *   when conf is NULL).  No workspace: the softmax is recomputed from conf.
 *   priors, arm_loc, loc, loc_t and grad_loc must be 16-byte aligned (read / written as 16-byte vectors; TDRN_E_ARG
 *   otherwise, before anything is enqueued); every other pointer needs only its element alignment.
 *   Errors before any launch: TDRN_E_ARG (null pointer, bad size), TDRN_E_WORKSPACE, TDRN_E_UNSUPPORTED.  No allocation, no
 *   host synchronisation, no float atomics: every sum runs in a fixed order, so results are bitwise reproducible.
 * ====================================================================================== */
/* encode alone (box_utils.py:151-172, the arithmetic tdrn_match uses): matched (P,4) point form, priors (P,4) center-size,
 * out (P,4); all three 16-byte aligned (TDRN_E_ARG otherwise). */
TDRN_API int tdrn_encode(const float *matched, const float *priors, int P, float var0, float var1, float *out, void *stream);
TDRN_API size_t tdrn_match_workspace_bytes(int B, int P, int max_truths);
TDRN_API int tdrn_match(const float *truths, const int32_t *truth_off, int T_total, int max_truths, int B,
                        const float *priors, int P, const float *arm_loc, float threshold, float var0, float var1,
                        float *loc_t, int32_t *conf_t, void *workspace, size_t workspace_bytes, void *stream);
TDRN_API size_t tdrn_multibox_loss_workspace_bytes(int B, int P, int C);
TDRN_API int tdrn_multibox_loss_forward(const float *loc, const float *conf, const float *loc_t, const int32_t *conf_t,
                                        int B, int P, int C, int negpos_ratio, float *loss_out, uint8_t *sel,
                                        int32_t *num_pos, void *workspace, size_t workspace_bytes, void *stream);
TDRN_API int tdrn_multibox_loss_backward(const float *loc, const float *conf, const float *loc_t, const int32_t *conf_t,
                                         const uint8_t *sel, const int32_t *num_pos, const float *grad_loss, int B,
                                         int P, int C, float *grad_loc, float *grad_conf, void *stream);

/* ========================================================================================
 * (ii-c) Training augmentation, SSDAugmentation on the device -- replaces
 *     SSDAugmentation(size, mean) = ConvertFromInts, ToAbsoluteCoords, PhotometricDistort, Expand(mean), RandomSampleCrop,
 *     RandomMirror, ToPercentCoords, Resize(size), SubtractMeans(mean)         utils/augmentations.py:618-635
 *   followed by VOCDetection.pull_item's BGR -> RGB and HWC -> CHW (data/voc0712.py:379-382), for a whole batch of raw
 *   uint8 frames, in two launches and with no host synchronisation.  The draws are consumed in the reference's order
 *   (augmentations.py:188-198, :544-551, :144-156, :418-442, :237-311, :485-491); semantics are the reference's, quirks
 *   included:
 *   - every image goes through the fp32 BGR -> HSV -> BGR round trip (cv2's float path: h in [0, 360], s and v unscaled),
 *     with contrast before it or after it; brightness adds, contrast and saturation multiply, hue adds and wraps
 *     (> 360 -> -360, < 0 -> +360), no clamp anywhere.  Off values are exact no-ops (x * 1, x + 0; hue 0 never wraps);
 *   - lighting noise permutes the channels: canvas channel c = distorted channel perm[c];
 *   - Expand: a draw of 1 means NO expand.  The canvas is int(h*r) x int(w*r), filled with mean[c] in canvas channel c
 *     (the mean is not permuted with the image); the image sits at (int(left), int(top)); boxes shift by those ints;
 *   - RandomSampleCrop: the IoU test never rejects (max_iou is inf), so the five non-None modes sample alike.  left =
 *     uniform(W - w) and top = uniform(H - h) are one-argument calls (low = W - w, high = 1.0): the left edge lies in
 *     [1, W - w] when W - w >= 1.  A trial is kept when some box centre lies strictly inside the int rect; kept boxes are
 *     clamped to it and shifted.  Boxes move in fp64 and are cast to fp32 at the end;
 *   - Resize is cv2.resize INTER_LINEAR on fp32: source coordinate (d + 0.5) * (n_src / n_dst) - 0.5 in double, cast to
 *     float, floor, border clamp as tdrn_preprocess_u8; weights (1 - f, f) in fp32, horizontal pass then vertical, unfused.
 *   Deviations, by design:
 *   - the reference draws new crop modes without bound; here at most TDRN_AUGMENT_MAX_ROUNDS, then no crop and status bit
 *     TDRN_AUGMENT_CROP_FALLBACK;
 *   - an image with no truths gets no crop (the reference never augments one: voc0712.py:360-369);
 *   - the random source is Philox4x32-10, keyed by the 64-bit seed, counter (draw slot, 0, sample id): a sample's result
 *     depends on (seed, sample id) alone, not on B or its place in the batch.  The <= 50 crop trials of a mode round run on
 *     a wave's lanes and the lowest passing trial wins, which has the sequential loop's distribution.  uniform(lo, hi) =
 *     lo + (hi - lo) * u with a 53-bit u; randint(n) = (32-bit word * n) >> 32.
 *   - tape mode instead replays recorded draws (randint results and uniform results, in the reference's order) one by one:
 *     the exact decisions of the reference for its own RandomState.  A tape that runs out ends the crop (no crop), draws
 *     0 from then on and sets TDRN_AUGMENT_TAPE_EXHAUSTED.
 *
 * tdrn_augment_sample: one launch.  hw (B,2) int32 DEVICE [h, w] per image; truths (T_total,5) fp64 DEVICE rows [x1,y1,x2,
 *   y2,label] as fractions, image b = rows [truth_off[b], truth_off[b+1]) with truth_off (B+1) int32 DEVICE, at most
 *   max_truths (<= TDRN_AUGMENT_MAX_TRUTHS, else TDRN_E_UNSUPPORTED) per image (offsets that break the promise are clamped).
 *   Exactly one source: sample_ids (B) int64 DEVICE with `seed` (Philox), or tape (fp64 DEVICE) with tape_off (B+1) int32
 *   DEVICE (image b replays tape[tape_off[b] .. tape_off[b+1])); both or neither -> TDRN_E_ARG.
 *   Writes params (B) records, out_truths (T_total,5) fp32 rows [x1,y1,x2,y2,label] (fractions of the output) packed with
 *   out_off (B+1) int32 -- the truth layout tdrn_match reads; T_total and max_truths of the input remain valid bounds for
 *   it.  Rows behind out_off[B] are not written.
 * tdrn_augment_apply: images (B) DEVICE table of {HWC uint8 BGR frame, h, w} (rows of 3*w bytes); params as written by
 *   tdrn_augment_sample; mean (3) HOST floats (BGR); out (B,3,S,S) fp32 = resized - mean, channels RGB when to_rgb,
 *   fully overwritten.  Only pixels inside a frame are read, whatever the params say.  S <= TDRN_AUGMENT_MAX_SIZE.
 *   Errors before any launch: TDRN_E_ARG (null pointer, bad size, no or two sources), TDRN_E_UNSUPPORTED.  No allocation,
 *   no host synchronisation, no workspace.
 * ====================================================================================== */
#define TDRN_AUGMENT_MAX_TRUTHS 512
#define TDRN_AUGMENT_MAX_ROUNDS 32
#define TDRN_AUGMENT_MAX_SIZE 2048
#define TDRN_AUGMENT_CROP_FALLBACK 1     /* status bits */
#define TDRN_AUGMENT_TAPE_EXHAUSTED 2
typedef struct {
    float brightness;        /* added (0 = off) */
    float contrast_pre;      /* multiplied before the HSV round trip (1 = off) */
    float contrast_post;     /* multiplied after it (1 = off) */
    float saturation;        /* multiplies s (1 = off) */
    float hue;               /* added to h, then wrapped (0 = off) */
    int32_t perm[3];         /* canvas channel c = distorted channel perm[c] */
    int32_t canvas_w, canvas_h, img_x, img_y;          /* expand canvas and the frame's place on it (no expand: w, h, 0, 0) */
    int32_t crop_x0, crop_y0, crop_x1, crop_y1;        /* crop rect on the canvas (no crop: the canvas) */
    int32_t cropped;         /* 1: a crop trial was kept and its centre test chose the boxes */
    int32_t mirror;
    int32_t kept;            /* boxes out */
    int32_t status;          /* TDRN_AUGMENT_* bits */
} tdrn_augment_params;
typedef struct {
    const uint8_t *data;     /* HWC uint8 BGR, rows of 3 * w bytes */
    int32_t h, w;
} tdrn_augment_image;
TDRN_API int tdrn_augment_sample(const int32_t *hw, const double *truths, const int32_t *truth_off, int T_total, int max_truths,
                                 int B, uint64_t seed, const int64_t *sample_ids, const double *tape, const int32_t *tape_off,
                                 tdrn_augment_params *params, float *out_truths, int32_t *out_off, void *stream);
TDRN_API int tdrn_augment_apply(const tdrn_augment_image *images, const tdrn_augment_params *params, int B, const float *mean,
                                int S, int to_rgb, float *out, void *stream);

/* ========================================================================================
 * (ii-d) Training augmentation for TRN pairs, pairSSDAugmentation on the device -- replaces, for a batch of raw frames,
 *     VOCDetection.pull_translational_item's translated second frame and truths            data/voc0712.py:400-458
 *     pairSSDAugmentation(size, mean) = pairPhotometricDistort, pairExpand(mean), pairRandomSampleCrop, pairRandomMirror,
 *     then per frame percent coordinates, cv2.resize and the mean                          utils/augmentations.py:637-689
 *   in two launches and with no host synchronisation.  A pair is a frame (frame 0) and a second frame (frame 1) of the same
 *   size under shared decisions; everything section (ii-c) says holds, and on top of it:
 *   - Translation (only when the caller supplies no second frame, for an image with truths), r = max_trans_ratio: for
 *     attempt a = 1, 2, 3 draw u_x = rand(), then u_y = rand(); x_trans = (-r / a) + ((u_x * 2) * r) / a, y_trans alike;
 *     add x_trans to columns 0 and 2 of the truths and y_trans to columns 1 and 3; the attempt is accepted when every box
 *     centre (x1 + x2) / 2, (y1 + y2) / 2 lies strictly inside (0, 1) on both axes.  On accept the pixel shift is
 *     trans_x = int(x_trans * W), trans_y = int(y_trans * H) (truncated toward zero) while the boxes move by the fraction
 *     itself -- the reference's mismatch, kept -- and the moved truths are clipped to [0, 1].  After three failures frame 1
 *     is a copy of frame 0, its truths are frame 0's, unclipped, and status gets TDRN_AUGMENT_TRANS_FALLBACK;
 *   - frame 1 is cv2.warpAffine(frame 0, [[1,0,tx],[0,1,ty]]) on uint8: dst(x, y) = src(x - tx, y - ty), 0 outside.  The
 *     black border belongs to the frame: it goes through the photometric distortion like any pixel, and only places
 *     outside the frame's rect on the expand canvas get the mean;
 *   - the photometric, expand and mirror draws and their order are section (ii-c)'s; one set of values serves both frames;
 *     canvas and mirror width come from frame 0;
 *   - a crop trial is kept when some index i has the centre of box i of frame 0 AND the centre of box i of frame 1 strictly
 *     inside the int rect; that one mask selects the kept rows of both frames (the same count), each set is clamped to the
 *     rect and shifted.
 *   Deviations, by design: those of (ii-c); an image with no truths gets no translation either (attempts = 0, frame 1 =
 *   frame 0); Philox: the shared decisions use the slots of tdrn_augment_sample, so for one (seed, sample id) the embedded
 *   record's photometric, expand and mirror fields equal that entry's; the translation attempts take slots 16-21 (attempt a:
 *   16 + 2(a-1) for u_x, the next for u_y), which tdrn_augment_sample never draws.  Tape mode replays the translation's
 *   rand() values first (two per attempt made), then the chain's.
 *
 * tdrn_augment_pair_sample: one launch.  hw, truths, truth_off, T_total, max_truths, B, seed, sample_ids, tape, tape_off as
 *   tdrn_augment_sample.  truths_t NULL: frame 1's truths are made by the translation rule.  truths_t (T_total,5) fp64
 *   DEVICE: frame 1's rows under the same offsets (the same count per image), used as they are; no translation, no
 *   translation draws, attempts = 0.  max_trans_ratio outside [0, 1) -> TDRN_E_ARG.  Writes params (B) pair records and two
 *   packed row sets out_truths, out_truths_t (T_total,5) fp32 behind the one out_off (B+1) int32.
 * tdrn_augment_pair_apply: one launch.  images as tdrn_augment_apply.  images_t NULL: frame 1 is frame 0 read at
 *   (x - trans_x, y - trans_y), 0 outside.  images_t (B) DEVICE table: the second frames (the same sizes; a pixel outside a
 *   smaller one reads as 0) and trans_x, trans_y are ignored.  out, out_t (B,3,S,S) fp32, both fully overwritten.  Only
 *   pixels inside a frame are read, whatever the records say.  Limits and errors as tdrn_augment_apply.
 *   No allocation, no host synchronisation, no workspace in either entry.
 * ====================================================================================== */
#define TDRN_AUGMENT_TRANS_FALLBACK 4    /* status bit: three translation attempts failed, frame 1 is a copy */
typedef struct {
    tdrn_augment_params base;        /* the shared decisions; kept counts either frame's rows */
    double shift_x, shift_y;         /* the accepted x_trans, y_trans (fractions added to the truths), else 0 */
    int32_t trans_x, trans_y;        /* the pixel shift int(x_trans * w), int(y_trans * h), else 0 */
    int32_t attempts;                /* translation attempts made: 1-3; 0 when frame 1 was supplied or there are no truths */
    int32_t reserved;
} tdrn_augment_pair_params;
TDRN_API int tdrn_augment_pair_sample(const int32_t *hw, const double *truths, const double *truths_t, const int32_t *truth_off,
                                      int T_total, int max_truths, int B, double max_trans_ratio, uint64_t seed,
                                      const int64_t *sample_ids, const double *tape, const int32_t *tape_off,
                                      tdrn_augment_pair_params *params, float *out_truths, float *out_truths_t,
                                      int32_t *out_off, void *stream);
TDRN_API int tdrn_augment_pair_apply(const tdrn_augment_image *images, const tdrn_augment_image *images_t,
                                     const tdrn_augment_pair_params *params, int B, const float *mean, int S, int to_rgb,
                                     float *out, float *out_t, void *stream);

/* PriorBox.forward -- layers/functions/prior_box.py:33-64 (host, double arithmetic, cast to
 * fp32, clamp).  aspect_ratios ragged: ar_count[k] values per map, concatenated in `ars`.
 * out == NULL: returns the number of priors only.  Returns P (>= 0) or a negative error. */
TDRN_API int tdrn_prior_box(int n_maps, const int *feature_maps, double image_size,
                            const double *steps, const double *min_sizes,
                            const double *max_sizes, int n_max_sizes, const int *ar_count,
                            const double *ars, int clip, int flip, float *out_host);

/* Detect.forward -- layers/functions/detection.py:25-70, fully on device, batched over
 * (image, class):  two-stage decode (:43-48), score > conf_thresh (:53), boxes*scale (:59),
 * cpu_nms semantics (:60), first top_k survivors packed as [score,x1,y1,x2,y2] (:61-63).
 *   loc (B,P,4)  conf (B*P,C)  priors (P,4)  arm_loc (B,P,4) or NULL  -- device fp32; loc, priors, arm_loc and the workspace
 *   must be 16-byte aligned (read / written as 16-byte vectors; TDRN_E_ARG otherwise, before anything is enqueued)
 *   scale: 4 HOST floats (the caller's [w,h,w,h]; evaluate.py:461)
 *   out (B,C,top_k,5) device fp32, fully overwritten (class 0 and unused slots = 0)
 *   counts_out (B*C) device int32 or NULL: survivors per (image,class), capped at top_k. */
/* Any P (no LDS-derived limit: the 1216-pixel scale of multi_eval.py:24 has P = 92055).
 * tdrn_detect_dev_scale: the same with `scale` as 4 DEVICE floats (16-byte aligned) -- evaluate.py:461 builds
 * the scale as a CUDA tensor; reading it on the device keeps the call free of host synchronisation. */
TDRN_API size_t tdrn_detect_workspace_bytes(int B, int P, int C, int top_k);
TDRN_API int tdrn_detect(const float *loc, const float *conf, const float *priors,
                         const float *arm_loc, const float *scale_host, int B, int P, int C,
                         int top_k, float conf_thresh, double nms_thresh, float *out,
                         int32_t *counts_out, void *workspace, size_t workspace_bytes,
                         void *stream);
TDRN_API int tdrn_detect_dev_scale(const float *loc, const float *conf, const float *priors,
                                   const float *arm_loc, const float *scale_dev, int B, int P, int C,
                                   int top_k, float conf_thresh, double nms_thresh, float *out,
                                   int32_t *counts_out, void *workspace, size_t workspace_bytes,
                                   void *stream);

/* Preprocess -- replaces base_transform + the channel swap of
 *     data/__init__.py:7-12 (cv2.resize(image,(S,S)) -> float32 -> -= mean) and data/voc0712.py:467-468
 *     (BGR -> RGB, HWC -> CHW); test_video.py:103-105 skips the swap (to_rgb = 0).
 *   frames (B, H0, W0, 3) uint8 BGR device; out (B, 3, S, S) fp32 NCHW device.
 *   Resize = OpenCV's INTER_LINEAR for 8-bit images (half-pixel centres, 11-bit fixed-point
 *   coefficients, uint8 result) restated from imgproc/resize.cpp; cv2 itself is not available in
 *   the build image, so this piece is "parity unpinned" by the reference: oracle.base_transform_u8 is
 *   pinned by hand-worked known-answer cases and by staying within one grey level of torch's independent floating-point
 *   bilinear (tests/test_oracle_pin.py); the device kernel is bit-exact against that oracle. */
TDRN_API int tdrn_preprocess(const uint8_t *frames, int B, int H0, int W0, int S, const float mean_bgr[3],
                             int to_rgb, float *out, void *stream);
/* The same resize, result left as cv2.resize returns it -- uint8 -- in planes: out (B, 3, S, S) uint8 device, channel-swapped when
 * to_rgb.  Together with tdrn_net_io.reserved[3] (below) this is SURVEY 8f rank 1 in full: the frame stays uint8 until the first conv's
 * loader reads it and subtracts the mean there ("fused into the first conv's loader"); no fp32 copy of the batch is ever written.
 * float(uint8) - mean is exact, so both routes give the net bit-identical inputs (tests/test_gpu_net.py). */
TDRN_API int tdrn_preprocess_u8(const uint8_t *frames, int B, int H0, int W0, int S, int to_rgb, uint8_t *out, void *stream);

/* ========================================================================================
 * (iii) Whole-network forward -- replaces build_net(...)/RefineSSD.forward:
 *     model/dualrefinedet_vggbn.py:10-117,119-206,217-222   (TDRN_DRN_VGGBN)
 *     model/dualrefinedet_mobilenet.py:8-125,127-199        (TDRN_DRN_MOBILENET)
 *     model/ssd4scale_mobile.py:9-84,86-140                 (TDRN_SSD4SCALE_MOBILE)
 *     model/refinedet_vgg.py:112-219                        (TDRN_REFINEDET_VGG)
 *     model/ssd4scale_vgg.py:71-135                         (TDRN_SSD4SCALE_VGG)
 * ====================================================================================== */
typedef enum {
    TDRN_DRN_VGGBN = 0,
    TDRN_DRN_MOBILENET = 1,
    TDRN_SSD4SCALE_MOBILE = 2,
    TDRN_REFINEDET_VGG = 3,
    TDRN_SSD4SCALE_VGG = 4
} tdrn_model;

typedef struct {
    int model;        /* tdrn_model                                                         */
    int size;         /* 320 or 512 (build_net rejects anything else)                       */
    int num_classes;  /* 21                                                                 */
    int c7_channel;   /* 1024                                                               */
    int def_groups;   /* deformable groups of the ODM heads (1)                             */
    int bn;           /* VGG trunk with BatchNorm                                           */
    int multihead;    /* 5x5 deformable heads summed with the 3x3 ones                      */
    int deform;       /* ssd4scale_*: deformable ARM heads (df_group = 8), TRN temporal net */
    int test_phase;   /* 1: softmax on conf (phase == 'test'); 0: raw logits                */
    int dtype;        /* tdrn_dtype of the dense path                                       */
    int use_refine;   /* refinedet_vgg: ARM loc heads present (4-tuple output)               */
    int plan_flags;   /* TDRN_PLAN_* bits; 0 = the default plan.  Two handles in one process may differ.   */
    int reserved[4];
} tdrn_net_config;

/* Plan-shaping switches (tdrn_net_config.plan_flags).  Every one of them changes the launch plan only: outputs are
 * bit-identical with the bit set or clear, except TDRN_PLAN_NO_DEFORM_TS in the 16-bit modes (where the rounding of the
 * deformable heads sits differently; both stay inside the 16-bit drift bounds of tests/test_gpu_net.py).
 * No environment variable overrides them. */
#define TDRN_PLAN_NO_FUSE_FIRST 1   /* keep the first conv a launch of its own (its output tensor is then materialised) */
#define TDRN_PLAN_NO_LATE_SIDE  2   /* release the side-lane convs on their true inputs instead of behind conv5_3      */
#define TDRN_PLAN_ONE_STREAM    4   /* no side lanes: every launch on the caller's stream                              */
#define TDRN_PLAN_NO_DEFORM_TS  8   /* deformable heads as the fused gather kernel (no transform-then-sample)           */
#define TDRN_PLAN_CHAIN         16  /* the small top-of-pyramid layers as ONE queue-driven launch (measured slower: off by default) */
/* Kernel-choice switches (tests/test_gpu_pin16.py holds the default plan bit-identical to each of them): */
#define TDRN_PLAN_NO_CONV_PP    32  /* conv3x3_pp.hip's layers stay on the loader/consumer kernel conv3x3_patch.hip                */
#define TDRN_PLAN_NO_PP_SK      64  /* conv3x3_pp.hip runs whole items only (no chained split)                                     */
#define TDRN_PLAN_NO_CONV_PATCH 128 /* neither 3x3 direct-conv kernel: every conv on the generic implicit GEMM (conv_igemm.hip)    */
#define TDRN_PLAN_DWPW          512 /* MobileNet trunks: eight conv_dw blocks as ONE launch each (dwpw.hip dwpw_kernel: the depthwise output stays in
                                       LDS; bit-identical; measured SLOWER than the two launches -- the depthwise conv on the vector ALU
                                       beside 128 live accumulators -- hence opt-in)                                                    */
#define TDRN_PLAN_NO_PW1X1      1024 /* the wide 1x1 convs stay on conv_igemm.hip instead of dwpw.hip's persistent GEMM (pw1x1_kernel)     */
#define TDRN_PLAN_NO_DW_SLIDE   2048 /* depthwise 3x3 layers on the one-row strip kernel instead of the sliding-window one (same bits)       */
#define TDRN_PLAN_DW_SLIDE_ALL  4096 /* ... the sliding-window kernel (8-row segments) at every batch, also where it leaves CUs idle       */
#define TDRN_PLAN_NO_CONV_WS    8192 /* the pooled Cin = 64 layer (conv1_2, with the first conv fused) stays on conv3x3_patch.hip instead of the weight-stationary conv3x3_ws.hip (conv2_1, full-resolution output, is on conv3x3_patch.hip either way) */
#define TDRN_PLAN_NO_YGEMM_V2  16384 /* transform-then-sample heads: the transform on the round-3 schedule of ygemm_k256 (two barriers per tile, stores behind the
                                       multiply phase) instead of the round-5 one (deform.hip ygemm_k256_v2_kernel); same bits                    */
#define TDRN_PLAN_NO_HEAD3X3   32768 /* the narrow fp32 3x3 heads (ARM loc) stay on conv_igemm.hip instead of head3x3.hip (different K order: the fp32 sums
                                       differ in their last bits)                                                                        */
#define TDRN_PLAN_TS_ONE_RANGE  65536 /* transform-then-sample heads: the whole batch as ONE range (Y of the whole batch in its buffer) instead of ranges
                                       whose Y fits the memory-side cache (192 MiB); same bits -- for tools and tests that read Y back       */
#define TDRN_PLAN_NO_PATCH_TAIL 131072 /* conv3x3_patch.hip and dwpw.hip pw1x1_kernel run whole items only: no 64- / 128-cout sub-items in an XCD's last, sparsely filled
                                        * round (the tail split of round 6: same MFMA rows, same K order -- bit-identical; for A/B runs and the test) */
#define TDRN_PLAN_FAULT_HANDOFF 256 /* fault injection (tests only): producers of the chained split never raise their flag, so the
                                       consumers' bounded polls run out -> the forward is reported failed, it does not hang          */

typedef struct tdrn_net tdrn_net;

/* Builds the layer plan on the host (no device work). */
TDRN_API int tdrn_net_create(const tdrn_net_config *cfg, tdrn_net **out);
/* Frees the host-side plan.  It does NOT destroy the HIP streams / events the net used: they go back to a per-process,
 * per-device pool and are reused by the next net on that device.  Reason (ROCm 7.2, csrc/dev/graph_destroy_repro.hip): a hipGraph
 * captured AFTER streams / events that took part in an earlier capture had been destroyed crashed inside hipGraphLaunch.
 * The caller must not destroy a net while a forward of it (or a graph captured from one) is still executing. */
TDRN_API void tdrn_net_destroy(tdrn_net *net);

/* state_dict interface: names and shapes are the reference's (entries ending in
 * num_batches_tracked are not parameters and are rejected with TDRN_E_PARAM).
 * tdrn_net_param_count/info enumerate what the plan expects: the reference's names and shapes, in the order the plan
 * consumes them (load by name, as load_state_dict does; the order carries no meaning). */
TDRN_API int tdrn_net_param_count(const tdrn_net *net);
TDRN_API int tdrn_net_param_info(const tdrn_net *net, int index, const char **name,
                                 int64_t shape[4], int *ndim);
/* Copies one fp32 HOST tensor into the net's staging area. */
TDRN_API int tdrn_net_set_param(tdrn_net *net, const char *name, const float *data_host,
                                int64_t numel);

/* Device memory the caller must provide. */
TDRN_API size_t tdrn_net_weight_bytes(const tdrn_net *net);
TDRN_API size_t tdrn_net_workspace_bytes(const tdrn_net *net, int batch);
TDRN_API int tdrn_net_num_priors(const tdrn_net *net);

/* Folds BatchNorm into the preceding conv, repacks OIHW -> [Cout_pad][kh][kw][Cin] in the
 * net's dtype, and uploads the blob (synchronous; one-time).  Every expected parameter must
 * have been set.  Ranks that receive the blob by RCCL broadcast skip this call and use
 * tdrn_net_adopt_weights() instead. */
TDRN_API int tdrn_net_pack_weights(tdrn_net *net, void *weights_dev, size_t weights_bytes,
                                   void *stream);
TDRN_API int tdrn_net_adopt_weights(tdrn_net *net);

/* The outputs (arm_loc, odm_loc, conf, offsets[], loc_maps[]) may start at ANY 4-byte-aligned address: the same bits as at a
 * 16-byte-aligned one (the geometry alone chooses the kernels and their arithmetic; a 16-byte store becomes four 4-byte ones).
 * Each is written exactly over its own extent: (B,P,4) / (B*P,C) / (B,G*18,H,W) / (B,12,H,W) floats, nothing before or behind. */
typedef struct {
    const float *x;        /* (B,3,S,S) fp32 NCHW, mean-subtracted 0..255 range, device      */
    int batch;
    float *arm_loc;        /* (B,P,4) fp32; DRN/RefineDet: ARM loc; ssd4scale: the loc output */
    float *odm_loc;        /* (B,P,4) fp32; NULL for ssd4scale                               */
    float *conf;           /* (B*P,C) fp32 softmax (test phase) or logits                    */
    float *offsets[4];     /* optional (B,G*18,H,W) fp32 NCHW out (arm_offset_list); or NULL */
    const float *ref_loc[4]; /* ssd4scale deform=1: (B,12,H,W) fp32 NCHW loc maps IN        */
    float *loc_maps[4];    /* ssd4scale deform=0 ret_loc: (B,12,H,W) fp32 NCHW raw loc maps OUT */
    /* reserved[0] != NULL, ssd4scale deform=1 only: REUSE the deformable offsets the previous forward of this net computed in
     * this workspace at this batch size instead of recomputing them from ref_loc (the reference's cached offset_list of the frames
     * between two key frames, evaluate_trn.py:459-462: offsets are a function of the key frame's loc maps only).  ref_loc may then
     * be NULL; TDRN_E_STATE when no such forward came before (other workspace, other batch).
     * reserved[1] != NULL, ssd4scale deform=1 only: KEY-FRAME BROADCAST -- (intptr_t) reserved[1] = Bk, the number of key frames:
     * ref_loc (and the optional `offsets` outputs) hold Bk samples and frame b of the batch uses the offsets of key frame b % Bk,
     * i.e. the batch is n = B / Bk frames of each of Bk clips in frame-major order.  One forward then does what the reference's
     * loop does frame by frame with its cached offset_list (evaluate_trn.py:452-462): the frames of an interval depend on the key
     * frame only through those offsets.  TDRN_E_ARG unless 1 <= Bk <= B and B % Bk == 0.
     * reserved[2] != NULL, with ref_loc: a hipEvent_t that the stream producing the ref_loc maps (the static net's forward, running
     * on ANOTHER stream beside this one) records when they are complete.  The forward waits for it right before its first read of
     * ref_loc -- behind its trunk, which does not depend on the maps -- instead of the caller serialising the two forwards.
     * reserved[3] != NULL: a `const tdrn_u8_frames *` -- the batch as UINT8 planes instead of `x` (which may then be NULL): the input
     * of the net is float(planes[b][c][y][x]) - mean[c].  16-bit plans of the VGG trunks read the planes inside the first conv, which
     * is computed by conv1_2's producers (conv3x3_ws.hip); every other plan converts them with one small launch into a workspace
     * tensor first.  Same output bits as the fp32 route. */
    void *reserved[4];
} tdrn_net_io;
typedef struct {
    const uint8_t *planes; /* (B, 3, S, S) uint8, device, in the net's channel order (tdrn_preprocess_u8 with to_rgb as the driver swaps) */
    float mean[3];         /* per plane, i.e. in the SAME channel order (BGR means (104,117,123) become (123,117,104) behind to_rgb)      */
} tdrn_u8_frames;

TDRN_API int tdrn_net_forward(tdrn_net *net, const void *weights_dev, void *workspace,
                              size_t workspace_bytes, const tdrn_net_io *io, void *stream);

/* Device-side failures.  Two launches hand data between workgroups through flags with BOUNDED polls (the chained split of
 * conv3x3_pp.hip; the opt-in chain launch of conv_igemm.hip).  A poll that runs out never hangs the GPU and never passes
 * silently: the kernel stores a code into a host-visible (pinned, device-mapped) status word owned by the net.
 * tdrn_net_check returns TDRN_OK, or TDRN_E_DEVICE when any forward enqueued on this net SINCE THE LAST CHECK has reported such a
 * failure (the word is cleared by the call); it does not synchronise -- call it after the stream (or the hipGraph replay) that
 * ran the forward has been synchronised to learn about THAT forward.  tdrn_net_forward performs the same check on entry, so a
 * failed forward makes the next tdrn_net_forward on the net return TDRN_E_DEVICE instead of launching ("never continue after
 * an error"); the call after that runs again (flags and counters are re-zeroed by every forward).
 * `detail` (or NULL) receives the raw word: bit 0 chained-split poll of conv3x3_pp.hip, bit 1 chain-launch poll. */
TDRN_API int tdrn_net_check(tdrn_net *net, unsigned *detail);

/* Per-kernel accounting of the LAST forward for bench.py's roofline line: algorithmic FLOPs
 * and bytes per kernel family, and (when profiling is enabled) hipEvent-measured time.
 * tdrn_net_profile(net, 1) makes the next forwards record an event pair around every launch and run
 * everything on `stream` (no overlap: the kernel's own duration); tdrn_net_profile(net, 2) records the
 * same pairs on the production schedule (side lanes on: the duration a launch has in the real step).
 * Both add launch gaps: use only in a dedicated profiling pass. */
typedef struct {
    char name[48];
    int launches;
    double flops;        /* algorithmic FLOPs (2*MAC) of all launches                        */
    double bytes;        /* algorithmic HBM bytes (inputs + weights + outputs, once each)   */
    double ms;           /* summed launch durations (profiling on), else 0                   */
} tdrn_kernel_stat;
TDRN_API int tdrn_net_profile(tdrn_net *net, int enable);
TDRN_API int tdrn_net_kernel_stats(tdrn_net *net, tdrn_kernel_stat *out, int max_entries);
/* same accounting per launch of the last profiled forward (name = producing parameter / op kind) */
TDRN_API int tdrn_net_op_stats(tdrn_net *net, tdrn_kernel_stat *out, int max_entries);
/* the same launches as a timeline: start / end of every launch of the last profiled forward in ms after the first launch's
 * start, and the stream lane it ran on (0 = the caller's stream); entry i corresponds to entry i of tdrn_net_op_stats */
TDRN_API int tdrn_net_op_timeline(tdrn_net *net, float *start_ms, float *end_ms, int *lane, int max_entries);

/* Test / debug access to the plan's internal activation tensors (NHWC, net dtype) after a
 * forward on the same workspace: tdrn_net_tensor_info names tensor `index` after the parameter
 * that produced it (e.g. "backbone.3", "L2Norm_4_3", "pool:backbone.3"); tdrn_net_read_tensor
 * converts it to fp32 NCHW (B,C,H,W) into out_dev.  Used by tests/ to compare every stage with
 * the oracle; not part of the hot path.  Tensors that a fused launch never materialises are not written: full-resolution
 * maps whose only reader is a fused max-pool, and -- in the 16-bit plans of the VGG trunks -- the first conv's output, which is
 * computed inside the next conv's loader (TDRN_PLAN_NO_FUSE_FIRST keeps it as its own launch). */
/* The plan's ops (test / debug access, like the tensors): what each launch computes and on which tensors, so that a test can
 * recompute ANY stage from the stage's own materialised input (tests/test_gpu_pin16.py: every conv of the 16-bit plans against an
 * fp64 convolution of its device input with the 16-bit-rounded folded weights).  Tensor fields are indices for
 * tdrn_net_tensor_info / tdrn_net_read_tensor, -1 = none. */
typedef struct {
    int kind;          /* 0 first conv (Cin = 3), 1 dense conv, 2 ConvTranspose2d(2,2), 3 depthwise 3x3, 4 MaxPool2d(2,2), 5 L2Norm,
                          6 1x1 offset conv, 7 deformable heads (loc + conf of one pyramid level), 8 anything else            */
    int in, out, res;  /* input, output (-1: a head that writes arm_loc / odm_loc / conf), residual added before the ReLU       */
    int pool;          /* conv: output of the MaxPool2d(2,2) fused into this launch (then `out` is not materialised), or -1    */
    int off, y;        /* deformable heads: the fp32 offset tensor; the transform GEMM's output Y (16-bit one-group plans) or -1 */
    int k, stride, pad, dil, relu, ceil_mode, splitk, groups;
    int out_kind;      /* 0 tensor, 1 arm_loc, 2 odm_loc, 3 conf                                                               */
    int level;         /* heads / offset convs: pyramid level                                                                  */
    int n_branches, k2, pad2, off_c0[2]; /* deformable heads: 3x3 (+ 5x5) branch, first offset channel of each branch          */
    int y_tap_major;   /* deformable heads with y >= 0: 1 = Y is [tap][B*H*W][80], 0 = [B*H*W][y channels] (column of tap t: (t/3)*256 + (t%3)*80) */
    int fused_first;   /* conv: 1 = this launch also computes the first conv (its `in` is then not materialised)               */
    int fused_dw;      /* depthwise: 1 = this launch also computes the pointwise conv behind it (dwpw.hip: its `out` is not materialised
                          and the next op, that conv, is not a launch of its own); conv: 1 = computed by the depthwise op in front   */
    char w[48], b[48], bn[48], w2[48], b2[48];  /* state_dict prefixes ('' = none): weight / bias owner / BatchNorm; second source (merged 5x5+3x3 heads; offset2;
                          deformable heads: w = 3x3 loc, b = 3x3 conf, w2 = 5x5 loc, b2 = 5x5 conf)                             */
    int y_groups;      /* deformable heads with y >= 0: output-column groups of <= 80 (12 loc + 3 * classes conf columns; 21 classes: 1,
                          31: 2, 81: 4).  Tensor y holds one region per group, y channels / y_groups channels each; group g's region
                          starts g * (y channels / y_groups) * H * W * B elements into the buffer and holds columns [80 g, 80 g + 80)   */
} tdrn_op_info;
TDRN_API int tdrn_net_op_count(const tdrn_net *net);
TDRN_API int tdrn_net_op_info(const tdrn_net *net, int index, tdrn_op_info *out);

TDRN_API int tdrn_net_tensor_count(const tdrn_net *net);
TDRN_API int tdrn_net_tensor_info(const tdrn_net *net, int index, const char **label, int *C, int *H,
                                  int *W);
TDRN_API int tdrn_net_read_tensor(const tdrn_net *net, const void *workspace, int batch, int index,
                                  float *out_dev, void *stream);
/* The inverse, and a forward that starts in the middle of the plan -- analysis only (scripts/attribution.py: which stage's
 * 16-bit rounding moves a detection): tdrn_net_write_tensor stores fp32 NCHW values (B,C,H,W) into tensor `index` of the
 * workspace, rounded once to the net dtype; tdrn_net_forward_from runs the plan's ops [first_op, end) assuming everything the
 * earlier ops produce (workspace tensors, and the head outputs in `io` that earlier ops wrote) is already in place.  Needs a
 * TDRN_PLAN_ONE_STREAM plan (TDRN_E_STATE otherwise: the side lanes' event graph assumes a whole forward). */
TDRN_API int tdrn_net_write_tensor(const tdrn_net *net, void *workspace, int batch, int index,
                                   const float *in_dev, void *stream);
TDRN_API int tdrn_net_forward_from(tdrn_net *net, const void *weights_dev, void *workspace,
                                   size_t workspace_bytes, const tdrn_net_io *io, int first_op, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* TDRN_HIP_H */
