/* qd_infer_conv.h -- C ABI of libqd_infer_conv.so: the 2-D convolution of nn.Conv2d computed straight from the packed low-bit
 * weights of a quantized student, with fp32 matrix instructions on the MI355X (gfx950).
 *
 * qd_infer.h gave nn.Linear and nn.Embedding a form that is read from bits / 8 bytes per weight; qd_infer_mm.h the Linear layer
 * for many rows of x.  This library does the same for a convolution, as an implicit GEMM: the packed weights of 16 output
 * channels are decoded once per 256 output pixels and multiplied with v_mfma_f32_16x16x4_f32 against input windows that are
 * gathered from x on the fly -- no im2col matrix and no fp32 weight tensor ever exist in memory.  It is an artifact of its own,
 * as the other two are: this header and libqd_infer_conv.so, and nothing of the other libraries.
 *
 * The format and the weight value are those of qd_infer.h ("The format is ...", "The weight value.") for the contiguous weight
 * W[cout][cin][kh][kw] seen as the 2-D tensor [rows = cout][cols = cin kh kw]: the stream of qd_pack_uniform_f32, one
 * (alpha, beta) per FLAT bucket -- so the packed weight of a conv tensor is bit for bit what the training quantizer makes of that
 * tensor -- bucket == 0 or cout cols < bucket one bucket, 2 <= levels <= 256, 1 <= bits <= 8, levels <= 2^bits;
 * w = (((float)c / (float)(levels - 1)) alpha[k] + beta[k]) + 0.0f, bit for bit what qd_unpack_uniform_f32 writes.
 *
 * Geometry.  oh = (h + 2 pad_h - kh) / stride_h + 1, ow likewise; zero padding, dilation 1, groups 1.  Column k of the GEMM
 * is (ci kh + a) kw + b, the weight's own memory order, and the input element of output pixel (n, p, q) in that column is
 * x[n][ci][p stride_h - pad_h + a][q stride_w - pad_w + b], or the value 0.0f where that lies outside the image.
 *
 * The Conventions of qd_infer.h hold word for word for the one call here: device pointers, asynchronous on `stream`; `packed`,
 * alpha, beta, x, bias, y 4-byte aligned and no other alignment changes a bit of a result; writes exactly
 * y[0 .. batch cout oh ow), reads nothing outside packed[0 .. qd_packed_bytes(cout cols, bits)), alpha / beta[0 .. num_buckets),
 * x[0 .. batch cin h w), bias[0 .. cout) -- a padded position is NOT LOADED (it is not loaded and then masked); ONE kernel
 * launch, no workspace, no allocation, no synchronisation, so it can be recorded into a hipGraph (by-value arguments frozen at
 * record time, device memory read at replay time); batch == 0 or cout == 0 returns 0 without a launch; 0 on success, a positive
 * hipError_t if the launch failed, QDC_ERR_INVALID_ARGUMENT (-1) -- nothing written, nothing launched -- for a NULL required
 * pointer with a non-zero size, a misaligned pointer, a negative size, levels outside 2 .. 256, bits outside 1 .. 8,
 * levels > 2^bits, bucket < 0, kh, kw, stride_h or stride_w < 1, pad_h or pad_w < 0, h + 2 pad_h < kh or w + 2 pad_w < kw, or
 * cin kh kw, cout cin kh kw bits, the element count of x or the element count of y not fitting an int64.
 */
#ifndef QD_INFER_CONV_H
#define QD_INFER_CONV_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QDC_ABI_VERSION 1
#define QDC_ERR_INVALID_ARGUMENT (-1)

int qdc_abi_version(void);          /* QDC_ABI_VERSION */
const char* qdc_target_arch(void);  /* "gfx950" */
const char* qdc_error_string(int code);

/* Test hook, as qdm_set_grid_cap of qd_infer_mm.h: at most `blocks` blocks per launch of this library, so that the later
 * trips of the kernel's loop over tiles run at small shapes.  Process-wide, a plain int: set it before launching, not
 * concurrently.  Returns the previous cap; 0 (or any value < 1) means no cap and is what a fresh library has. */
int qdc_set_grid_cap(int blocks);

/* Convolution: y[n][co][p][q] = sum_k xwin[n][p][q][k] w[co][k] (+ bias[co]), k = (ci kh + a) kw + b over K = cin kh kw columns
 * (Geometry above).  `bias` may be NULL.
 * Arithmetic, all fp32.  Every output element has ONE accumulator that starts at +0.0f and is carried through
 * v_mfma_f32_16x16x4_f32 instructions, each of which adds four products w[co][k] xwin[k] to it.  The columns are taken in
 * slabs of 64, front to back; inside a slab in groups of 16, front to back; inside the group that starts at column g the four
 * instructions take the columns g + jj + {0, 4, 8, 12}, jj = 0, 1, 2, 3.  A last slab of fewer than 64 columns runs only the
 * groups that hold a column; the columns of such a group past K enter as 0 x 0, and a padded input enters as 0 x w.  The bias
 * is added last, one fp32 addition.
 * This order is a function of cin kh kw ALONE: it does not depend on the batch, on where the pixel sits in its image or in
 * the call, on the stride or the padding, on cout, bucket, levels, bits or the grid cap; there is no split over K and there
 * are no atomics, so image n of a batched call has the bits of the call on that image alone, and the same call gives the same
 * bits every time.
 * Bound: |y - exact| <= 1e-6 (sum_k |x w| + |bias|).  How the matrix unit rounds inside an instruction, and what it makes of
 * subnormal operands, products and sums, is the hardware's: for those this header promises the bound, not bits.  Where every
 * partial sum is exactly representable the result is exact, whatever the order.
 * A NaN or inf weight of channel co reaches every y[:, co] (0 x inf = NaN, through the padding too) and no other channel; a NaN
 * or inf in x reaches the outputs whose window holds it, and no other.
 * Index width: x and y are addressed with 32-bit offsets where each holds fewer than 2^31 elements, with 64-bit offsets
 * otherwise; the choice is made on the host and changes no bit of a result. */
int qdc_conv2d_packed_f32(const uint8_t* packed, const float* alpha, const float* beta,
                          int64_t cout, int64_t cin, int kh, int kw, int64_t bucket, int levels, int bits,
                          const float* x /* [batch][cin][h][w] */, int64_t batch, int64_t h, int64_t w,
                          int stride_h, int stride_w, int pad_h, int pad_w,
                          const float* bias /* [cout] or NULL */, float* y /* [batch][cout][oh][ow] */, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* QD_INFER_CONV_H */
