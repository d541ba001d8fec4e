/* qd_infer_gru.h -- C ABI of libqd_infer_gru.so: one step of a GRU (nn.GRUCell, or one time step of one layer and direction of
 * nn.GRU) computed straight from the packed low-bit recurrent weights of a quantized student, with fp32 matrix instructions on
 * the MI355X (gfx950).
 *
 * qd_infer_rnn.h gave the LSTM step a form that is read from bits / 8 bytes per weight.  A GRU step is not that step with a gate
 * removed: the reset gate multiplies the RECURRENT half of the candidate, n = tanh(gi_n + r gh_n) with b_hn inside the product,
 * so the two products W_ih x and W_hh h must stay two sums and cannot be carried through one accumulator.  This library gathers
 * the three gate rows of a unit into four rows of an MFMA tile (the fourth is idle), computes gi = x W_ih^T and gh = h W_hh^T as
 * two sums of their own in the same registers one after the other and finishes the step (two sigmoids, tanh, h') in the lane that
 * holds all six: one launch per step, no [batch, 3 hidden] round trip through memory.  It is an artifact of its own, as the other
 * four are: this header and libqd_infer_gru.so, and nothing of the other libraries.
 *
 * The format and the weight value are those of qd_infer.h ("The format is ...", "The weight value.") for each of the two
 * contiguous weights on its own, W_ih[3 hidden][input] and W_hh[3 hidden][hidden]: the stream of qd_pack_uniform_f32, one
 * (alpha, beta) per FLAT bucket counted per weight tensor -- bit for bit what the training quantizer makes of weight_ih_l* /
 * weight_hh_l* and of a cell's weights, each quantized as its own tensor -- bucket == 0 or fewer elements than a bucket one
 * bucket, 2 <= levels <= 256, 1 <= bits <= 8, levels <= 2^bits; w = (((float)c / (float)(levels - 1)) alpha[k] + beta[k]) + 0.0f,
 * bit for bit what qd_unpack_uniform_f32 writes.  The rows are in torch's order: gate g (0 = r, 1 = z, 2 = n) of hidden unit j is
 * row g hidden + j, of the weights, of the biases, of `pre` and of each half of `gates` alike.
 *
 * The Conventions of qd_infer.h hold for the one call here: device pointers, asynchronous on `stream`; every pointer 4-byte
 * aligned and no other alignment changes a bit of a result; writes exactly h_out[0 .. batch hidden) and, where given,
 * gates[0 .. batch 2 3 hidden); reads nothing outside the two streams, their alpha / beta[0 .. num_buckets), x[0 .. batch input) or
 * pre[0 .. batch 3 hidden), h[0 .. batch hidden) and the biases[0 .. 3 hidden); ONE kernel launch, no workspace, no allocation, no
 * synchronisation, no atomics, no wait of one block for another, so it can be recorded into a hipGraph (by-value arguments
 * frozen at record time, device memory read at replay time).  A sequence of T steps is T calls.  batch == 0 or hidden == 0
 * returns 0 without a launch; 0 on success, a positive hipError_t if the launch failed, QDG_ERR_INVALID_ARGUMENT (-1) --
 * nothing written, nothing launched -- for: levels outside 2 .. 256, bits outside 1 .. 8, levels > 2^bits or bucket < 0 of a
 * weight that is used; a negative size; a misaligned pointer; 3 hidden, a weight's element or bit count, batch 2 3 hidden or
 * batch input not fitting an int64; both or neither of x and pre; bias_ih together with pre; a NULL pointer where an array with
 * elements is needed (h, h_out; W_hh's three; in cell mode W_ih's three where input > 0); h_out == h.
 */
#ifndef QD_INFER_GRU_H
#define QD_INFER_GRU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QDG_ABI_VERSION 1
#define QDG_ERR_INVALID_ARGUMENT (-1)

int qdg_abi_version(void);          /* QDG_ABI_VERSION */
const char* qdg_target_arch(void);  /* "gfx950" */
const char* qdg_error_string(int code);

/* Test hook, as qdm_set_grid_cap of qd_infer_mm.h: at most `blocks` blocks per launch of this library, so that the later
 * trips of the kernel's loop over tiles run at small shapes.  Process-wide, a plain int: set it before launching, not
 * concurrently.  Returns the previous cap; 0 (or any value < 1) means no cap and is what a fresh library has. */
int qdg_set_grid_cap(int blocks);

/* One GRU step for `batch` rows.  Exactly one of x and pre is given.
 * Cell mode (x): gi[b][r] = sum_k x[b][k] W_ih[r][k], r < 3 hidden, then gi + bias_ih[r]; gh[b][r] = sum_k h[b][k] W_hh[r][k], then
 *   gh + bias_hh[r].  A bias that is NULL adds nothing (no addition is made).
 * Pre mode (pre): gi[b][r] = pre[b][r], the input projection with bias_ih already in it (qdm_linear_packed_f32 over all time
 *   steps at once); the six W_ih arguments and `input` are not looked at and may be NULL / 0, bias_ih must be NULL.  gh as in
 *   cell mode.
 * Epilogue, fp32, one rounded operation at a time, per unit j with the rows r = j, z = hidden + j, n = 2 hidden + j:
 *   r = 1.0f / (1.0f + expf(-(gi_r + gh_r))), z = 1.0f / (1.0f + expf(-(gi_z + gh_z))), n = tanhf(gi_n + r gh_n) (bias_hh's third
 *   part is inside gh_n and so inside the product, as in torch), h' = (1.0f - z) n + z h (a subtraction, two products, one
 *   addition).  `gates`, where given, receives per batch row gi[0 .. 3 hidden) and then gh[0 .. 3 hidden) as they enter the epilogue.
 *   expf and tanhf are the device library's: this header promises h' to the float64 epilogue of the fp32 gi and gh within
 *   40.2 x 2^-24 (|h| + 1) -- four times the 10.06 units the fp32 reference formulas reach on the host, where half an ulp of r
 *   enters tanhf's argument times gh_n; the kernel reaches 3.94 (tests/test_hip_packed_gru.py, profiles/packed_gru_error.txt) --,
 *   not bits across compiler releases.
 * Arithmetic of gi and gh, all fp32.  Each of the two has an accumulator of its OWN that starts at +0.0f and is carried through
 *   v_mfma_f32_16x16x4_f32 instructions, each of which adds four products to it, as qdm_linear_packed_f32 takes a weight of that
 *   many columns (slabs of 64 front to back, groups of 16 front to back, inside the group at column g the four instructions take
 *   g + jj + {0, 4, 8, 12}; a last slab of fewer than 64 columns runs only the groups that hold a column, the columns of such a
 *   group past the end enter as 0 x 0).  The two sums are never added before the epilogue.  The order of gi is a function of
 *   `input` ALONE and that of gh of `hidden` ALONE: not of batch, of where a row sits in the batch, of bucket, levels, bits or the
 *   grid cap.  Row b of a call has the bits of the call on that row alone, and the same call gives the same bits every time.
 * Bound: |gi - exact| <= 1e-6 (sum |terms| + |bias_ih|), gh likewise; where every partial sum is exactly representable they are
 *   exact.  How the matrix unit rounds inside an instruction, and what it makes of subnormals, is the hardware's.
 * A NaN or inf weight in row r reaches gi[:, r] or gh[:, r] (0 x inf = NaN) and through it h' of that unit, and no other unit; a
 *   non-finite activation propagates as IEEE arithmetic does through the weight rows.  The tile's idle fourth row is never read:
 *   no value that is not a sum over a real weight row reaches an output.
 * Aliasing.  h_out must NOT overlap h anywhere: every block reads all of h[b] for its rows b while other blocks write h_out.
 *   h_out == h is refused; any other overlap is the caller's error and gives unspecified values in h_out (never an access
 *   outside the arrays).  `gates` must not overlap any input. */
int qdg_gru_cell_packed_f32(
    const uint8_t* packed_ih, const float* alpha_ih, const float* beta_ih, int64_t bucket_ih, int levels_ih, int bits_ih, /* W_ih [3 hidden][input] */
    const uint8_t* packed_hh, const float* alpha_hh, const float* beta_hh, int64_t bucket_hh, int levels_hh, int bits_hh, /* W_hh [3 hidden][hidden] */
    int64_t hidden, int64_t input,
    const float* x /* [batch][input], or NULL: pre mode */, const float* pre /* [batch][3 hidden], or NULL: cell mode */,
    const float* h /* [batch][hidden] */, int64_t batch,
    const float* bias_ih /* [3 hidden] or NULL */, const float* bias_hh /* [3 hidden] or NULL */,
    float* h_out /* [batch][hidden] */, float* gates /* [batch][2][3 hidden] or NULL */,
    void* stream);

#ifdef __cplusplus
}
#endif

#endif /* QD_INFER_GRU_H */
