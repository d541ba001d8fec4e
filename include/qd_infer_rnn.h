/* qd_infer_rnn.h -- C ABI of libqd_infer_rnn.so: one step of an LSTM (nn.LSTMCell, or one time step of one layer and direction
 * of nn.LSTM) computed straight from the packed low-bit recurrent weights of a quantized student, with fp32 matrix instructions
 * on the MI355X (gfx950).
 *
 * qd_infer.h, qd_infer_mm.h and qd_infer_conv.h gave nn.Linear, nn.Embedding and nn.Conv2d a form that is read from bits / 8
 * bytes per weight.  An LSTM step is no Linear layer followed by element-wise operations: the four gate rows of one hidden unit
 * sit `hidden` rows apart in the weight, and the step has two weights over two inputs.  This library gathers the four rows of a
 * unit into one MFMA tile, carries both products through ONE accumulator and finishes the step (sigmoid, tanh, c', h') in the
 * lane that holds the four gates: one launch per step, no [batch, 4 hidden] round trip through memory.  It is an artifact of
 * its own, as the other three are: this header and libqd_infer_rnn.so, and nothing of the other libraries.
 *
 * The format and the weight value are those of qd_infer.h ("The format is ...", "The weight value.") for each of the two
 * contiguous weights on its own, W_ih[4 hidden][input] and W_hh[4 hidden][hidden]: the stream of qd_pack_uniform_f32, one
 * (alpha, beta) per FLAT bucket counted per weight tensor -- bit for bit what the training quantizer makes of weight_ih_l* /
 * weight_hh_l* and of a cell's weights, each quantized as its own tensor -- bucket == 0 or fewer elements than a bucket one
 * bucket, 2 <= levels <= 256, 1 <= bits <= 8, levels <= 2^bits; w = (((float)c / (float)(levels - 1)) alpha[k] + beta[k]) + 0.0f,
 * bit for bit what qd_unpack_uniform_f32 writes.  The rows are in torch's order: gate g (0 = i, 1 = f, 2 = g, 3 = o) of hidden
 * unit j is row g hidden + j, of the weights, of the biases, of `pre` and of `gates` alike.
 *
 * The Conventions of qd_infer.h hold for the one call here: device pointers, asynchronous on `stream`; every pointer 4-byte
 * aligned and no other alignment changes a bit of a result; writes exactly h_out[0 .. batch hidden), c_out[0 .. batch hidden) and,
 * where given, gates[0 .. batch 4 hidden); reads nothing outside the two streams, their alpha / beta[0 .. num_buckets),
 * x[0 .. batch input) or pre[0 .. batch 4 hidden), h and c[0 .. batch hidden) and the biases[0 .. 4 hidden); ONE kernel launch, no
 * workspace, no allocation, no synchronisation, no atomics, no wait of one block for another, so it can be recorded into a
 * hipGraph (by-value arguments frozen at record time, device memory read at replay time).  A sequence of T steps is T calls.
 * batch == 0 or hidden == 0 returns 0 without a launch; 0 on success, a positive hipError_t if the launch failed,
 * QDR_ERR_INVALID_ARGUMENT (-1) -- nothing written, nothing launched -- for: levels outside 2 .. 256, bits outside 1 .. 8,
 * levels > 2^bits or bucket < 0 of a weight that is used; a negative size; a misaligned pointer; 4 hidden, a weight's element
 * or bit count, batch 4 hidden or batch input not fitting an int64; both or neither of x and pre; bias_ih together with pre; a NULL
 * pointer where an array with elements is needed (h, c, h_out, c_out; W_hh's three; in cell mode W_ih's three where input > 0);
 * h_out == h.
 */
#ifndef QD_INFER_RNN_H
#define QD_INFER_RNN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QDR_ABI_VERSION 1
#define QDR_ERR_INVALID_ARGUMENT (-1)

int qdr_abi_version(void);          /* QDR_ABI_VERSION */
const char* qdr_target_arch(void);  /* "gfx950" */
const char* qdr_error_string(int code);

/* Test hook, as qdm_set_grid_cap of qd_infer_mm.h: at most `blocks` blocks per launch of this library, so that the later
 * trips of the kernel's loop over tiles run at small shapes.  Process-wide, a plain int: set it before launching, not
 * concurrently.  Returns the previous cap; 0 (or any value < 1) means no cap and is what a fresh library has. */
int qdr_set_grid_cap(int blocks);

/* One LSTM step for `batch` rows.  Exactly one of x and pre is given.
 * Cell mode (x): a[b][r] = sum_k x[b][k] W_ih[r][k] + sum_k h[b][k] W_hh[r][k], r < 4 hidden, then (a + bias_ih[r]) + bias_hh[r];
 *   a bias that is NULL adds nothing (no addition is made).
 * Pre mode (pre): pre[b][r] is the input projection with bias_ih already in it (qdm_linear_packed_f32 over all time steps at
 *   once); the six W_ih arguments and `input` are not looked at and may be NULL / 0, bias_ih must be NULL.  a[b][r] is the
 *   W_hh sum alone, then (a + pre[b][r]) + bias_hh[r].
 * Epilogue, fp32, one operation at a time: i, f, o = 1.0f / (1.0f + expf(-a)), g = tanhf(a_g), c' = f c + i g (two products,
 *   one addition), h' = o tanhf(c').  `gates`, where given, receives the four pre-activations a of every unit as they enter the
 *   epilogue.  expf and tanhf are the device library's: this header promises h' and c' to the float64 epilogue of the fp32
 *   gates within 16.4 x 2^-24 and 11.5 x 2^-24 (|c| + 1) (tests/test_hip_packed_lstm.py), not bits across compiler releases.
 * Arithmetic of a, all fp32.  Every a[b][r] has ONE accumulator that starts at +0.0f and is carried through
 *   v_mfma_f32_16x16x4_f32 instructions, each of which adds four products to it: first the columns of W_ih against x, then
 *   the columns of W_hh against h, each part as qdm_linear_packed_f32 takes a weight of that many columns (slabs of 64 front to
 *   back, groups of 16 front to back, inside the group at column g the four instructions take g + jj + {0, 4, 8, 12}; a last
 *   slab of fewer than 64 columns runs only the groups that hold a column, the columns of such a group past the end enter as
 *   0 x 0).  A slab never holds columns of both parts.  The order is a function of `input` and `hidden` ALONE: not of batch, of
 *   where a row sits in the batch, of bucket, levels, bits or the grid cap.  Row b of a call has the bits of the call on that
 *   row alone, and the same call gives the same bits every time.
 * Bound: |a - exact| <= 1e-6 (sum |terms| + |biases| + |pre|); where every partial sum is exactly representable a is exact.  How
 *   the matrix unit rounds inside an instruction, and what it makes of subnormals, is the hardware's.
 * A NaN or inf weight in row r reaches a[:, r] (0 x inf = NaN) and through it h' and c' of that unit, and no other unit.
 * Aliasing.  c_out may be c: each element is read and then written by the same lane.  h_out must NOT overlap h anywhere:
 *   every block reads all of h[b] for its rows b while other blocks write h_out.  h_out == h is refused; any other overlap is
 *   the caller's error and gives unspecified values in h_out (never an access outside the arrays).  `gates` must not overlap
 *   any input. */
int qdr_lstm_cell_packed_f32(
    const uint8_t* packed_ih, const float* alpha_ih, const float* beta_ih, int64_t bucket_ih, int levels_ih, int bits_ih, /* W_ih [4 hidden][input] */
    const uint8_t* packed_hh, const float* alpha_hh, const float* beta_hh, int64_t bucket_hh, int levels_hh, int bits_hh, /* W_hh [4 hidden][hidden] */
    int64_t hidden, int64_t input,
    const float* x /* [batch][input], or NULL: pre mode */, const float* pre /* [batch][4 hidden], or NULL: cell mode */,
    const float* h /* [batch][hidden] */, const float* c /* [batch][hidden] */, int64_t batch,
    const float* bias_ih /* [4 hidden] or NULL */, const float* bias_hh /* [4 hidden] or NULL */,
    float* h_out /* [batch][hidden] */, float* c_out /* [batch][hidden] */, float* gates /* [batch][4 hidden] or NULL */,
    void* stream);

#ifdef __cplusplus
}
#endif

#endif /* QD_INFER_RNN_H */
