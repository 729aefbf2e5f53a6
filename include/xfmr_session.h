/*
 * xfmr_session.h -- the session encoder of libxfmr_hip.so: append events to cached histories, one token per step.
 *
 * The serving path of the reference (xfmr_rec/service.py: recommend_with_query -> Model.embed) encodes a user's whole
 * history at every call. The encoder it builds is causal (BertConfig(is_decoder=True), xfmr_rec/models.py:355) with
 * absolute positions: row t of token_embeddings depends on rows 0 .. t only, and no earlier row changes when an event is
 * appended. These entries keep every layer's K and V per session, so an append runs ONE row through the Linears and one
 * query row against the session's cached keys. Conventions as in xfmr_hip.h: caller-owned device buffers, work enqueued on
 * `stream`, no HIP object created (a sequence of calls can be captured), 0 or a negative XFMR_E* code returned.
 * XFMR_ABI_VERSION stays 3: no struct of xfmr_hip.h changes.
 *
 * The cfg: hidden, heads, inter, layers, max_pos, precision, ln_eps describe the model as for xfmr_encoder_infer; every slot
 * holds max_len = max_pos rows. batch and seq_len are checked as there (positive, seq_len <= max_pos) and not read
 * otherwise. Refused before anything is launched: XFMR_ENC_BIDIRECTIONAL (XFMR_EUNSUPPORTED: an append changes every
 * earlier row there), non-zero dropout (XFMR_EINVAL), seq_offsets / row_pos / packed_rows set (XFMR_EINVAL: these entries
 * have their own row arrays), head size not 32 / 64 and more than 64 layers (XFMR_EUNSUPPORTED), misaligned buffers
 * (XFMR_EALIGN), a state or workspace smaller than the size query's bytes (XFMR_EWORKSPACE).
 *
 * Session state: ONE caller-owned device buffer of xfmr_session_state_bytes(cfg, n_slots) bytes that the library carves:
 *   - per (slot, layer, head) one contiguous panel [K: max_len x head_size | V: max_len x head_size], position-major, so a
 *     query streams it with coalesced 16-byte loads; the element type follows cfg.precision (fp32 / bf16);
 *   - per slot max_len key-mask bytes (1 = the item's table row has a non-zero element, as xfmr_embed_ln_fwd derives it);
 *   - per slot max_len last-layer token rows, fp32 (what xfmr_session_pool pools);
 *   - under bf16 storage the bf16 copy of the flat parameter buffer, made ONCE by xfmr_session_init: an append of a few rows
 *     is bound by reading the weights once, and xfmr_encoder_infer's per-call conversion would double that.
 */
#ifndef XFMR_SESSION_H
#define XFMR_SESSION_H

#include "xfmr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of the state for n_slots sessions / of the scratch of one xfmr_session_append call of up to max_rows rows.
 * 0: the cfg (or n_slots / max_rows <= 0) is refused. */
size_t xfmr_session_state_bytes(const xfmr_encoder_cfg* cfg, int32_t n_slots);
size_t xfmr_session_workspace_bytes(const xfmr_encoder_cfg* cfg, int64_t max_rows);

/* What the attend kernel does for this cfg, as integers, touching no device: out[0] = the key chunk C (keys one wave takes per
 * online-softmax step), out[1] = lanes per key (each reads 16 bytes), out[2] = keys per wave load, out[3] = bytes per K/V
 * element, out[4] = bf16 activation storage (qkv / ctx and the parameter copy), out[5] = max_len, then zeros. Returns the
 * code the other entries return for the cfg. */
int xfmr_session_plan(const xfmr_encoder_cfg* cfg, int32_t out[8]);

/* Carve the state, zero every mask byte and (bf16 storage) convert the parameters. Call it again after the weights change:
 * every slot is empty afterwards. */
int xfmr_session_init(const xfmr_encoder_cfg* cfg, const float* params, void* state, size_t state_bytes, int32_t n_slots,
                      void* stream);

/* Run n_rows NEW tokens through the encoder: row r is item item_idx[r] at position row_pos[r] of slot row_slot[r]. One call
 * serves the one-token step (one row per active session) and chunked prefill (consecutive positions of a slot): per layer
 * the rows' K and V are stored first (one launch), then every (row, head) attends to its slot's keys 0 .. pos (a second
 * launch), so a row of a chunk sees the keys the same call wrote. Keys beyond pos are never read, cached keys whose mask
 * byte is 0 are skipped, a query with no visible key gets ctx = 0. The Linears and LayerNorms are the forward-only forms of
 * xfmr_encoder_infer on n_rows rows. tok_out (n_rows, H) or NULL: the rows' last-layer outputs, which are also stored in
 * the state. A row whose slot is outside [0, n_slots) or whose position is outside [0, max_pos) stores nothing and gets a
 * zero tok_out row (a caller error is clamped, never a fault). No (slot, position) pair may occur twice in one call, and a
 * row at position p expects positions 0 .. p - 1 of its slot written by this or an earlier call (the caller's contract).
 * workspace: xfmr_session_workspace_bytes(cfg, max_rows >= n_rows) bytes, scratch of this call only. */
int xfmr_session_append(const xfmr_encoder_cfg* cfg, const float* params, void* state, size_t state_bytes, int32_t n_slots,
                        const int64_t* item_idx, const int32_t* row_slot, const int32_t* row_pos, int64_t n_rows,
                        const float* table, int64_t n_table_rows, float* tok_out, void* workspace, size_t workspace_bytes,
                        void* stream);

/* xfmr_pool's four rules (+ xfmr_l2_normalize_fwd when normalize != 0) over the stored rows [0, lens[i]) of slot slots[i]
 * with the stored mask bytes: out (n, H). lens[i] <= 0 or a slot outside [0, n_slots) gives a zero row; lens[i] is
 * clamped to max_len. */
int xfmr_session_pool(const xfmr_encoder_cfg* cfg, const void* state, size_t state_bytes, int32_t n_slots,
                      const int32_t* slots, const int32_t* lens, int32_t n, int32_t mode, int32_t normalize, float eps,
                      float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* XFMR_SESSION_H */
