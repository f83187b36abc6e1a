/* lwm_hip.h -- C ABI of the MI355X-native LWM hot path (liblwm_hip.so).
 *
 * The reference (LargeWorldModel/LWM) has no FFI: its hot path sits behind
 * Python callables.  Each entry point below names the reference interface it
 * replaces; INTEGRATION.md shows the ctypes binding a maintainer would add.
 *
 * Conventions (all entry points):
 *   - plain pointers + sizes; no torch / HIP types in signatures
 *     (`stream` is a hipStream_t passed as void*; NULL = default stream);
 *   - every pointer is DEVICE memory owned by the caller; the library never
 *     allocates, frees or synchronises; kernels are enqueued on `stream`;
 *   - return 0 (LWM_OK) or a negative LWM_E* code; lwm_last_error() returns a
 *     thread-local message for the last failure on the calling thread;
 *   - no global mutable state; one host thread per device is the supported
 *     threading model.
 */
#ifndef LWM_HIP_H
#define LWM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LWM_OK 0
#define LWM_EINVAL (-1)       /* bad argument (null, misaligned, bad shape) */
#define LWM_EUNSUPPORTED (-2) /* valid but not implemented (e.g. head_dim != 128) */
#define LWM_ELAUNCH (-3)      /* HIP reported a launch error */

/* A [B, S, H, D] tensor with D contiguous; strides in ELEMENTS.  This is the
 * reference's q/k/v layout: heads are split by reshape, not transposed
 * (lwm/llama.py:434-438), and shard_map hands the op (B, S/sp, H/tp, D) blocks
 * (lwm/llama.py:559-566). */
typedef struct LwmTensor4 {
    void* ptr;
    int64_t stride_b, stride_s, stride_h;
} LwmTensor4;

/* One ring step of blockwise attention: local queries [q_start, q_start+Sq)
 * against the K/V block holding global positions [k_start, k_start+Sk).
 *
 * Replaces: ringattention(q,k,v,attn_bias,segment_ids, axis_name="sp",
 *   float32_logits=True, blockwise_kwargs=dict(causal_block_size=1, ...))
 *   -- call site lwm/llama.py:539-569 -- and its custom-VJP backward.
 * Mask semantics (lwm/llama.py:425, :527-537, :546, :572-592):
 *   visible(q,k) = (k_pos <= q_pos if causal) AND segment_ids_q[q]==segment_ids_k[k]
 *                  AND key_valid[k] != 0
 *   (attn_bias in the reference is the key-padding mask turned into
 *   {0, finfo.min}; key_valid is that mask before the transform).
 * Rows with no visible key produce out = 0, lse = -inf.
 * Scores are q.k * scale in f32; softmax and all accumulators are f32
 * (float32_logits=True, lwm/llama.py:543); operands are bf16; D must be 128.
 */
#define LWM_MAX_PIECES 8
typedef struct LwmAttnArgs {
    LwmTensor4 q, k, v;    /* bf16 in */
    LwmTensor4 out;        /* bf16: fwd writes it when final_out; bwd reads it */
    float* lse;            /* [B,H,Sq] natural-log LSE: fwd writes when final_out; bwd reads */
    float* out_acc;        /* [B,Sq,H,D] f32 dense ring carry (normalised partial out) */
    float* lse_acc;        /* [B,H,Sq]   f32 ring carry */
    LwmTensor4 dout;       /* bf16 in (bwd) */
    LwmTensor4 dq, dk, dv; /* bf16 out (bwd, when final_out) */
    float* delta;          /* backward row statistics, lwm_attn_bwd_delta_bytes(B,H,Sq) bytes, written by
                            * lwm_attn_bwd_delta from out, dout and lse, read by lwm_attn_bwd_dq / _dkdv: per (b,h)
                            * [-lse*log2(e) | -rowsum(dout*out)], each row padded to a multiple of 64 queries */
    float* dq_acc;         /* [B,Sq,H,D] f32 dense carry */
    float* dk_acc;         /* [B,Sk,H,D] f32 dense carry (travels with the K/V block) */
    float* dv_acc;
    const int32_t* segment_ids_q; /* [B,Sq] or NULL */
    const int32_t* segment_ids_k; /* [B,Sk] or NULL (both or neither) */
    const uint8_t* key_valid;     /* [B,Sk] or NULL */
    int32_t B, H, Sq, Sk, D;
    int64_t q_start, k_start; /* global token position of local row 0 */
    float scale;              /* 1/sqrt(D) in the reference */
    int32_t causal;
    int32_t carry_in;  /* 1: merge with the *_acc carries before writing */
    int32_t final_out; /* 1: write bf16 out/lse (fwd) or dq / dk,dv (bwd); 0: write *_acc */
    /* Forward only -- the dense-mask / decode flavour (ringattention_inference,
     * lwm/llama.py:571-614): an arbitrary boolean mask (B,1,Q,K) as u8, combined
     * (AND) with the masks above; element (b,q,k) of THIS K/V block is
     * dense_mask[b*mask_stride_b + q*mask_stride_q + k].  NULL = none. */
    const uint8_t* dense_mask;
    int64_t mask_stride_b, mask_stride_q;
    /* Forward only -- split-K ("flash decoding") for short query blocks: the key
     * range is cut into k_splits contiguous pieces, each handled by its own
     * workgroups; piece s writes its normalised partial to
     * out_acc + s*B*Sq*H*D and lse_acc + s*B*H*Sq (requires final_out = 0,
     * carry_in = 0); merge with lwm_attn_combine.  0 or 1 = no split. */
    int32_t k_splits;
    /* Optional: block-sparsity hints for packed sequences.  seg_blocks_q [B][ceil(Sq/32)][2]
     * and seg_blocks_k [B][ceil(Sk/32)][2] hold the (min, max) segment id of every 32-row
     * block (filled by lwm_attn_segment_blocks; padded keys excluded).  When both are given
     * a workgroup only walks the tiles of the other operand whose segment range meets its
     * own -- whole documents of a packed batch are skipped instead of computed and masked.
     * Results are unchanged (the per-element mask is still applied).  NULL = no skipping. */
    const int32_t* seg_blocks_q;
    const int32_t* seg_blocks_k;
    /* lwm_attn_bwd_dq: 0 = dq_acc is [B,Sq,H,D], 1 = head-major [B,H,Sq,D]. */
    int32_t dq_acc_head_major;
    /* Piecewise position maps (lwm_version() >= 500; *_pieces = 0 or 1: one piece, the fields above say everything).
     * A shard under zigzag ownership is TWO runs of consecutive positions (half-chunks r and 2n-1-r), under a balanced
     * ownership of packed documents a few more, and so is the K/V a rank has gathered from its peers (what lies below its
     * first run, between its runs ...).  With q_pieces = P > 1:
     *   query rows [q_piece_row[i], q_piece_row[i+1]) sit at positions q_piece_pos[i] + (row - q_piece_row[i]),
     *   q_piece_row[0] = 0, q_piece_pos[0] = q_start, the last piece ends at Sq;  keys likewise.
     * One launch then covers what took one launch per (q segment, k segment) pair, with no carry in between -- at small
     * shards (S = 32768 over 8 ranks: 2048-row half-chunks) the pair launches cannot fill 256 CUs.  Requirements:
     * P <= LWM_MAX_PIECES; piece rows are multiples of 256, strictly ascending, inside (0, S); positions ascend with the
     * row and pieces do not overlap (pos[i+1] >= pos[i] + row[i+1] - row[i]).  Training kernels only (lwm_attn_fwd
     * without dense_mask / k_splits, lwm_attn_bwd_dq / _dkdv); results are bitwise those of the single-piece launch on the
     * same rows when the pieces happen to be adjacent. */
    int32_t q_pieces, k_pieces;
    int32_t q_piece_row[LWM_MAX_PIECES], k_piece_row[LWM_MAX_PIECES];
    int64_t q_piece_pos[LWM_MAX_PIECES], k_piece_pos[LWM_MAX_PIECES];
    /* Size in bytes of the buffer behind `delta`, or 0 = not given.  When given, lwm_attn_bwd_delta / _dq / _dkdv
     * refuse a buffer smaller than lwm_attn_bwd_delta_bytes(B,H,Sq) instead of overrunning it (the layout of the
     * statistics changed at lwm_version() 400: a [B,H,Sq] buffer of earlier versions is too small). */
    int64_t delta_bytes;
    /* dS hand-over (lwm_version() >= 610), backward only, optional: a workspace of lwm_attn_bwd_ds_bytes(...) bytes,
     * 16-byte aligned.  lwm_attn_bwd_dkdv then also stores the dS it computes (bf16, in a layout private to the two
     * kernels), and lwm_attn_bwd_dq called AFTERWARDS on the same stream with the same arguments computes
     * dq = scale * dS k from it in one GEMM instead of recomputing S and dP: 7 GEMM units per pair instead of 9.
     * dk and dv are bitwise what they are without it; dq differs in rounding only (its dS comes from the dK/dV kernel's
     * chains).  Honoured when lwm_attn_bwd_ds_bytes is not 0 for the call and the call has bf16 operands, no
     * segment ids, no key_valid, final_out = 1, carry_in = 0 and one piece per operand; any other call ignores the
     * workspace and runs as without it.  A workspace that is too small or misaligned for an eligible call: LWM_EINVAL,
     * nothing is launched.  NULL = no hand-over. */
    void* ds_ws;
    int64_t ds_ws_bytes;
} LwmAttnArgs;

int lwm_attn_fwd(const LwmAttnArgs* args, void* stream);
/* The backward of one ring step = three launches (no atomics, bit-reproducible): the row statistics once per query
 * block, then dq (a workgroup owns 128 queries and streams K/V: 3 GEMM units) and dk, dv (a workgroup owns 128 keys
 * and streams Q/dO: 4 units) per (query block, K/V block) pair, chained through the f32 carries.  [A form that
 * computed S and dP once and summed bf16 dq partials -- 5 units -- was measured in rounds 2-3 and retired in round 4:
 * profiles/r04_backward.md.] */
int lwm_attn_bwd_delta(const LwmAttnArgs* args, void* stream);
int lwm_attn_bwd_dq(const LwmAttnArgs* args, void* stream);
int lwm_attn_bwd_dkdv(const LwmAttnArgs* args, void* stream);

/* Bytes of the backward's row statistics (LwmAttnArgs::delta) for a [B, Sq, H, D] query block. */
int64_t lwm_attn_bwd_delta_bytes(int32_t B, int32_t H, int32_t Sq);
/* Exact bytes of the dS hand-over workspace (LwmAttnArgs::ds_ws) of one (query block, K/V block) pair, or 0 when the
 * shape is not eligible (Sq % 64, Sk % 128) or there is nothing to hand over.  Only the (64 queries x 32 keys) tiles
 * the dK/dV walk visits get room: causal, a tile wholly above the diagonal has none -- B * H * Sq * Sk bytes for a
 * causal square pair, twice that without the mask (32 GiB at B = 1, H = 32, Sq = Sk = 32768, causal). */
int64_t lwm_attn_bwd_ds_bytes(int32_t B, int32_t H, int32_t Sq, int32_t Sk, int32_t causal, int64_t q_start, int64_t k_start);

/* ------------------------------------------------------------------ the float32 flavour of the training op
 * The reference computes in `--dtype`, and its own default is fp32 (lwm/train.py:36; the launch scripts of
 * scripts/run_train_*.sh pass --dtype='fp32'; BASELINE configs[0] is the fp32 model).  These four entry points are
 * lwm_attn_fwd / lwm_attn_bwd_delta / _dq / _dkdv with FLOAT32 tensors behind every LwmTensor4 of LwmAttnArgs
 * (q, k, v, out, dout, dq, dk, dv: f32, D contiguous, strides in elements and multiples of 4; lse, the carries and the
 * row statistics are what they are in the bf16 flavour, and the statistics buffer has the same size).  Same mask
 * semantics, same carries (carry_in / final_out), same "rows with no visible key give 0 / -inf"; every contraction runs
 * on the exact-f32 matrix instruction (v_mfma_f32_32x32x2_f32), no operand is rounded to bf16.  Not taken:
 * piecewise position maps (q_pieces / k_pieces > 1), dense_mask, k_splits -> LWM_EUNSUPPORTED; the block-sparsity
 * hints are accepted and not read.  Kernels: lwm_amd/csrc/attn_f32.h. */
int lwm_attn_fwd_f32(const LwmAttnArgs* args, void* stream);
int lwm_attn_bwd_delta_f32(const LwmAttnArgs* args, void* stream);
int lwm_attn_bwd_dq_f32(const LwmAttnArgs* args, void* stream);
int lwm_attn_bwd_dkdv_f32(const LwmAttnArgs* args, void* stream);
/* The steps either side of the op at dtype = fp32 (lwm_amd/csrc/elem_f32.h): lwm_rope_bf16 / lwm_rmsnorm_{fwd,bwd}_bf16 /
 * lwm_swiglu_{fwd,bwd}_bf16 / lwm_softmax_ce_bf16 with float tensors (rows of C % 4 == 0, V % 4 == 0, n % 4 == 0, 16-byte
 * aligned), same arithmetic minus the roundings to bf16 (at dtype = f32 the reference's casts are identities,
 * lwm/llama.py:339-341); lwm_rmsnorm_bwd_f32 takes lwm_rmsnorm_bwd_workspace_bytes(rows, C) bytes of workspace.
 * lwm_sum_f32: dst = ((srcs[0] + srcs[1]) + ...) in argument order -- lwm_sum_f32_to_bf16 with a float result (the
 * owner-side reduction of returned dK / dV partials when the operands are f32). */
int lwm_rope_f32(LwmTensor4 x, LwmTensor4 y, const float* table, const int32_t* pos, int32_t B, int32_t S, int32_t H,
                 int32_t D, int32_t max_pos, int32_t conj, void* stream);
int lwm_rmsnorm_fwd_f32(const float* x, const float* w, float* y, float* rstd, int64_t rows, int32_t C, float eps,
                        void* stream);
int lwm_rmsnorm_bwd_f32(const float* x, const float* w, const float* g, const float* rstd, float* dx, float* dw,
                        void* workspace, int64_t rows, int32_t C, void* stream);
int lwm_swiglu_fwd_f32(const float* a, const float* b, float* y, int64_t n, void* stream);
int lwm_swiglu_bwd_f32(const float* a, const float* b, const float* g, float* da, float* db, int64_t n, void* stream);
int lwm_softmax_ce_f32(const float* logits, const int32_t* target, const float* weight, float* nll, int32_t* correct,
                       float* dlogits, int64_t rows, int32_t V, void* stream);
int lwm_sum_f32(const float* const* srcs, int32_t n_src, float* dst, int64_t n, void* stream);

/* ------------------------------------------------------------------ the sequence ring
 * The exchange that lax.ppermute performs under ringattention (lwm/llama.py:539-569, SURVEY.md Appendix
 * A.1), driven from C: for ring step t rank r holds the K/V block of rank (r - t) mod n, runs the local
 * queries against it on the COMPUTE stream while the block travels on to rank r+1 and the next one arrives
 * from rank r-1 on the SIDE stream (grouped ncclSend / ncclRecv of RCCL over xGMI), hipEvents handing the
 * double buffer back and forth.  The backward rotates K, V and the f32 dK/dV carries of the block; after n
 * steps they are home.  Ownership is the reference's: rank r holds positions [r*c, (r+1)*c) (contiguous,
 * lwm/llama.py:560-562); attn_bias / segment_ids are replicated, full length (lwm/llama.py:563-564).
 *
 * A ring object holds no device memory: the caller passes a workspace of lwm_ring_workspace_bytes()
 * bytes (K/V double buffer, f32 carries, mask slices), which must stay untouched until the compute stream
 * has passed the call.  Transports:
 *   lwm_ring_create            an existing ncclComm_t of the "sp" group (RCCL is resolved at run time:
 *                              dlsym in the process, else dlopen librccl.so -- the library has no link-time
 *                              dependency on it);
 *   lwm_ring_create_from_id    the library creates (and owns) the communicator from an ncclUniqueId
 *                              (lwm_ring_unique_id on rank 0, broadcast by the host's own means);
 *   lwm_ring_create_transport  any send/recv pair given as function pointers (tests drive the schedule
 *                              through it with in-process mailboxes; n = 1 needs no transport at all).
 */
typedef struct LwmRing LwmRing;

typedef struct LwmRingTransport {
    void* ctx;
    int (*group_start)(void* ctx);
    /* enqueue on `stream` (a hipStream_t): send `bytes` bytes at `buf` to ring rank `peer` / receive from it */
    int (*send)(void* ctx, const void* buf, int64_t bytes, int32_t peer, void* stream);
    int (*recv)(void* ctx, void* buf, int64_t bytes, int32_t peer, void* stream);
    int (*group_end)(void* ctx);
} LwmRingTransport;

typedef struct LwmRingArgs {
    LwmTensor4 q, k, v;      /* local shards [B,c,H,D] bf16; k and v dense (they are sent as they are) */
    LwmTensor4 out;          /* fwd: written; bwd: read */
    float* lse;              /* [B,H,c] f32: fwd writes, bwd reads */
    LwmTensor4 dout;         /* bwd in */
    LwmTensor4 dq, dk, dv;   /* bwd out, [B,c,H,D] bf16 */
    const int32_t* segment_ids; /* [B,S_global] or NULL -- replicated, full length */
    const uint8_t* key_valid;   /* [B,S_global] or NULL */
    int32_t B, c, H, D;      /* c = local sequence length = S_global / n */
    float scale;
    int32_t causal;
    void* workspace;         /* lwm_ring_workspace_bytes(B, c, H, D, backward, n, schedule) bytes, 256-byte aligned */
    int32_t layout;          /* LWM_RING_LAYOUT_*: which positions a rank owns */
    int32_t schedule;        /* LWM_RING_SCHEDULE_*: how K/V and the dK/dV contributions move */
    /* LWM_RING_LAYOUT_TABLE: HOST array of n_chunks = n * P ints (1 <= P <= LWM_MAX_PIECES): the sequence is cut into
     * n_chunks equal chunks, chunk j (positions [j * S/n_chunks, (j+1) * S/n_chunks)) belongs to rank chunk_owner[j]; every
     * rank owns exactly P chunks and holds them in ascending position order in its local rows.  Ignored otherwise. */
    const int32_t* chunk_owner;
    int32_t n_chunks;
    /* Gathered form only (lwm_ring_last_form): a caller-owned device buffer of lwm_ring_kv_keep_bytes() bytes that the
     * FORWARD gathers the fetched K/V into (instead of its workspace) and that the BACKWARD of the same layer, handed the
     * same buffer with kv_kept = 1, reads instead of fetching K/V again: a quarter of the bytes a layer moves over xGMI
     * (K/V twice + f32 partials once -> K/V once + partials), for (n - 1) * c * H * D * 4 bytes per layer kept between the
     * two calls -- 0.5 GB at S = 32768 over 8 ranks, 1.9 GB at S = 131072; 288 GB per GPU is what makes that a choice.
     * EVERY rank of the ring must make the same choice for a call (a rank that does not fetch does not send either).
     * NULL / 0 = fetch in both calls.  Ignored by the per-pair form. */
    void* kv_keep;
    int32_t kv_kept;
} LwmRingArgs;

/* Ownership.  CONTIGUOUS = the reference's: rank r holds positions [r*c, (r+1)*c) (lwm/llama.py:560-562).
 * ZIGZAG: rank r holds the half-chunks r and 2n-1-r (c/2 positions each, local rows [0,c/2) and [c/2,c)) -- the
 * permutation applied at the boundary that balances causal work: under contiguous ownership rank n-1 computes n
 * blocks and rank 0 one.  lse is an OPAQUE residual between lwm_ring_attn_fwd and _bwd of the same ring and geometry
 * (two dense [B,H,c/2] pieces, one per segment, or one [B,H,c] piece in local row order, as the form of the call has it);
 * everything else keeps its [B,c,H,D] shape in local row order. */
/* TABLE: any ownership of equal chunks, P per rank, handed over as LwmRingArgs::chunk_owner -- for packed batches, where
 * zigzag balances a full causal triangle but not documents: at BASELINE configs[4] (1,048,576 tokens in 15 documents, 8
 * ranks) the slowest zigzag rank computes 1.9x the mean; four chunks per rank assigned by visible-pair count (a loader
 * knows the document lengths: lwm_amd/ring.py balanced_layout) bring that to ~1.03.  Runs in the gathered form only
 * (lwm_ring_last_form): direct schedule, B = 1, causal, chunks of a multiple of 256 rows. */
enum { LWM_RING_LAYOUT_CONTIGUOUS = 0, LWM_RING_LAYOUT_ZIGZAG = 1, LWM_RING_LAYOUT_TABLE = 2 };
/* Exchange.  RING = the reference's (lax.ppermute i -> i+1): the K/V block, and in the backward its f32 dK/dV
 * carry, hop to the next rank once per step -- every byte crosses ONE link per step, n-1 (n) times.
 * DIRECT: MI355X's xGMI is a full mesh, so nothing is forwarded: one grouped exchange brings every rank exactly
 * the K/V segments its queries can see from their owners (all 7 links busy at once; zigzag + causal: 1/4 fewer
 * bytes than rotating whole blocks), and in the backward the f32 dK/dV partial of each remote block goes straight
 * back to its owner, which sums the <= n partials in a fixed order (lwm_sum_f32_to_bf16).  Results agree with RING
 * up to the f32 association of that sum. */
enum { LWM_RING_SCHEDULE_RING = 0, LWM_RING_SCHEDULE_DIRECT = 1 };

int lwm_ring_create(void* nccl_comm, int32_t rank, int32_t n, void* side_stream, LwmRing** out);
int lwm_ring_unique_id(void* id128);   /* 128 bytes = ncclUniqueId */
int lwm_ring_create_from_id(const void* id128, int32_t rank, int32_t n, void* side_stream, LwmRing** out);
int lwm_ring_create_transport(const LwmRingTransport* transport, int32_t rank, int32_t n, void* side_stream,
                              LwmRing** out);
int lwm_ring_destroy(LwmRing* ring);
int64_t lwm_ring_workspace_bytes(int32_t B, int32_t c, int32_t H, int32_t D, int32_t backward, int32_t n,
                                 int32_t schedule);
int lwm_ring_attn_fwd(LwmRing* ring, const LwmRingArgs* args, void* compute_stream);
int lwm_ring_attn_bwd(LwmRing* ring, const LwmRingArgs* args, void* compute_stream);
/* What ONE call of lwm_ring_attn_fwd (backward = 0) or lwm_ring_attn_bwd (backward = 1) makes rank `rank` send, in
 * bytes, under the given ownership and schedule -- a pure function of the geometry (no device is touched): the
 * forward's K/V, and in the backward the K/V again plus the f32 dK/dV carries (ring) or partials (direct). */
int64_t lwm_ring_planned_bytes(int32_t layout, int32_t schedule, int32_t n, int32_t rank, int32_t B, int32_t c, int32_t H,
                               int32_t D, int32_t causal, int32_t backward);
/* The same for LWM_RING_LAYOUT_TABLE (direct schedule, causal, B = 1 -- the form a table runs in): a rank sends each of its
 * chunks to every peer whose last chunk lies above it and, in the backward, returns an f32 dK and dV partial for every
 * chunk it fetched.  -1 for an unusable table. */
int64_t lwm_ring_planned_bytes_table(const int32_t* chunk_owner, int32_t n_chunks, int32_t n, int32_t rank, int32_t c, int32_t H,
                                     int32_t D, int32_t backward);
/* Size of LwmRingArgs::kv_keep for a shard shape: room for the K and the V rows of every other rank, (n - 1) * c rows each. */
int64_t lwm_ring_kv_keep_bytes(int32_t B, int32_t c, int32_t H, int32_t D, int32_t n);
/* bytes this ring object has sent since creation (diagnostic) */
int64_t lwm_ring_bytes_sent(const LwmRing* ring);
/* Which form the last lwm_ring_attn_fwd / _bwd call took (diagnostic): 0 = one launch per (q segment, k segment) pair,
 * chained through f32 carries; 1 = the GATHERED form of the direct schedule -- the fetched K/V segments laid down in
 * position order in one buffer and read through two-piece position maps (LwmAttnArgs::q_split / k_split): per kernel
 * two launches per call, the local block under the fetch and everything that arrived after it.  Taken when the call is
 * causal, B = 1, the K/V fetch is one group (lwm_ring_set_fetch_groups: the default) and every segment of a shard is a
 * multiple of 256 rows; same results up to f32 association (fewer carries: closer to the exact sum). */
int lwm_ring_last_form(const LwmRing* ring);
/* Direct schedule: the K/V fetch of a call goes out as `groups` grouped exchanges over contiguous ranges of rank distance,
 * nearest first, each with its own arrival event; step t of the schedule waits only for the group that holds distance t.
 * 1 (the default: one bulk-synchronous group keeps all xGMI links busy, and the kernels of the remote blocks run as ONE
 * launch per kernel over everything that arrived -- lwm_ring_last_form) ... n - 1 (every block is handed over as it lands, a
 * launch per block: for transports whose transfers are serial anyway, such as the IPC one).  Values above n - 1 mean n - 1. */
int lwm_ring_set_fetch_groups(LwmRing* ring, int32_t groups);
/* Diagnostic (rings created with LWM_RING_TIMING=1 in the environment: their events then carry timestamps): after the
 * last lwm_ring_attn_fwd / _bwd call has completed, the milliseconds from the call's entry to (kv_ms[t]) the arrival of
 * the K/V block of rank distance t (direct schedule, t >= 1) and to (kernels_ms[t]) the end of the kernels of step t;
 * count >= n entries each, -1 where undefined.  Blocks on the call's completion. */
int lwm_ring_fetch_timeline(LwmRing* ring, float* kv_ms, float* kernels_ms, int32_t count);
/* Diagnostic: ONE grouped exchange with ourselves through the ring's transport -- send `bytes` bytes at src to
 * our own ring rank and receive them into dst -- enqueued on the ring's side stream and handed over by the same
 * events an attention step uses (compute stream -> side stream -> compute stream).  With a ring made by
 * lwm_ring_create_from_id(n = 1) this is a complete first contact with RCCL on a single GPU: the run-time symbol
 * table, the by-value ncclUniqueId, ncclGroupStart / ncclSend / ncclRecv / ncclGroupEnd on a non-default stream. */
int lwm_ring_selftest(LwmRing* ring, const void* src, void* dst, int64_t bytes, void* compute_stream);

/* A transport that needs neither RCCL nor compute units: every rank owns a mailbox (device memory) that its peers map
 * through hipIpcMemHandles; a message is one hipMemcpyAsync into the receiver's mailbox (SDMA over xGMI between GPUs)
 * followed by a stream memory operation on an uncached flag word (hipStreamWriteValue32 / hipStreamWaitValue32), and
 * one local copy out of the mailbox on the receiving side.  All 256 CUs stay with the attention kernels, and because
 * IPC also works between processes sharing ONE GPU the complete multi-process driver can run on a single-GPU box.
 *   1. every rank: lwm_ring_ipc_export(rank, n, slot_bytes, slots, info, &ipc) -- allocates mailbox + flags on the
 *      current device; info receives lwm_ring_ipc_info_bytes() bytes to publish.  slot_bytes >= the largest message
 *      (a K/V or f32 dK/dV piece: B * c * H * D * 4 bytes covers everything the driver sends), slots >= 4 * B
 *      messages per ordered pair and group (8 is a good default); memory = n * slots * slot_bytes per rank.
 *   2. the host all-gathers the n info blobs by its own means (rank-major) -> lwm_ring_ipc_connect(ipc, all_infos).
 *   3. lwm_ring_create_ipc(ipc, side_stream, &ring) -- a ring object like any other; destroy the ring, then the ipc. */
typedef struct LwmRingIpc LwmRingIpc;
int64_t lwm_ring_ipc_info_bytes(void);
int lwm_ring_ipc_export(int32_t rank, int32_t n, int64_t slot_bytes, int32_t slots, void* info_out, LwmRingIpc** out);
int lwm_ring_ipc_connect(LwmRingIpc* ipc, const void* all_infos);
int lwm_ring_create_ipc(LwmRingIpc* ipc, void* side_stream, LwmRing** out);
int lwm_ring_ipc_destroy(LwmRingIpc* ipc);

/* (min, max) of segment_ids over each block of 32 rows, excluding rows whose valid[] is 0
 * (valid may be NULL); an all-invalid block gets (INT32_MAX, INT32_MIN).
 * blocks: [B][ceil(S/32)][2] int32. */
int lwm_attn_segment_blocks(const int32_t* segment_ids, const uint8_t* valid, int32_t* blocks,
                            int32_t B, int32_t S, void* stream);

/* Merge P normalised partial attention results (split-K pieces of one launch, or
 * the per-rank partials of a sequence-sharded K/V cache, lwm/llama.py:599-614):
 *   o_parts [P][B,Sq,H,D] f32, lse_parts [P][B,H,Sq] f32  ->
 *   out bf16 [B,Sq,H,D] (strided) if out.ptr != NULL, else out_f32 [B,Sq,H,D];
 *   lse [B,H,Sq] f32 (may be NULL).  Rows whose every partial is empty
 *   (lse = -inf) give out = 0, lse = -inf. */
int lwm_attn_combine(const float* o_parts, const float* lse_parts, int32_t P, LwmTensor4 out,
                     float* out_f32, float* lse, int32_t B, int32_t Sq, int32_t H, int32_t D,
                     void* stream);

/* KV-cache write (lwm/llama.py:440-492): cache[b, dst_row0 + i, :] = src[b, src_row0 + i, :]
 * for i < nrows; rows are row_elems bf16 (= H*D) contiguous; batch strides in
 * elements.  The caller decides which rows land in its shard (decode: only the
 * owning sp shard writes, :454-467). */
int lwm_kv_cache_write(void* cache, const void* src, int32_t B, int64_t cache_stride_b,
                       int64_t src_stride_b, int64_t dst_row0, int64_t src_row0, int64_t nrows,
                       int32_t row_elems, void* stream);

/* The same with the destination row read from DEVICE memory: row = *dst_row0_dev + row_offset + i;
 * rows outside [0, cache_rows) are skipped, which is the decode rule "only the owning sp shard
 * writes" (lwm/llama.py:454-467) with row_offset = -rank * cache_rows.  No host value changes from
 * one decode step to the next, so a step can be captured in a hipGraph and replayed. */
int lwm_kv_cache_write_at(void* cache, const void* src, int32_t B, int64_t cache_stride_b,
                          int64_t src_stride_b, const int32_t* dst_row0_dev, int64_t row_offset,
                          int64_t cache_rows, int64_t src_row0, int64_t nrows, int32_t row_elems,
                          void* stream);

/* ------------------------------------------------------------------ 8-bit KV cache (lwm_version() >= 520)
 * The cache as OCP e4m3fn bytes with one f32 scale per (row, head): 0.516 of the bf16 cache's bytes, in
 * memory and per decode step.  Per layer four tensors:
 *   cached_key, cached_value  uint8 (B, max_length, H, 128), the bits of e4m3fn, heads of a row contiguous;
 *   key_scale, value_scale    f32   (B, max_length, H).
 * One head of one row (128 bf16 values x): amax = max |x|; s = the smallest power of two with
 * amax / s <= 448, clamped to [2^-126, 2^127], s = 1 when amax == 0; q = e4m3(x / s), round to nearest even
 * (x / s is exact and in range: nothing saturates).  q * s is exactly representable in bf16.  Non-finite
 * inputs are not supported.
 *
 * lwm_kv8_cache_write / _at: the arguments of lwm_kv_cache_write / _at (row_elems = H * 128; cache strides in
 * bytes, src strides in bf16 elements) plus the scale tensor, its batch stride in floats, and H. */
int lwm_kv8_cache_write(void* cache, const void* src, int32_t B, int64_t cache_stride_b,
                        int64_t src_stride_b, int64_t dst_row0, int64_t src_row0, int64_t nrows,
                        int32_t row_elems, float* scale, int64_t scale_stride_b, int32_t H, void* stream);
int lwm_kv8_cache_write_at(void* cache, const void* src, int32_t B, int64_t cache_stride_b,
                           int64_t src_stride_b, const int32_t* dst_row0_dev, int64_t row_offset,
                           int64_t cache_rows, int64_t src_row0, int64_t nrows, int32_t row_elems,
                           float* scale, int64_t scale_stride_b, int32_t H, void* stream);

/* Cached-decode attention (one query per batch row) over that cache: the contract of lwm_attn_fwd's decode
 * case (Sq = 1, dense_mask, k_splits, final_out = 0).  The visible key range of each (B, Sk) mask row is
 * partitioned over k_splits pieces, one workgroup each; masked keys inside it contribute nothing whatever
 * their bytes and scales hold; the normalised partials out_acc [k_splits,B,1,H,D] f32 and lse_acc
 * [k_splits,B,H,1] f32 are merged by lwm_attn_combine; a row with nothing visible gives (0, -inf).
 * D = 128; q, the cache rows (k/v_stride_* in bytes) and out_acc 16-byte aligned; scale strides in floats, the
 * H scales of a row contiguous. */
typedef struct LwmKv8DecodeArgs {
    LwmTensor4 q;                   /* bf16 (B,1,H,D) */
    const void* k;                  /* e4m3 bytes (B,Sk,H,D) */
    const void* v;
    int64_t k_stride_b, k_stride_s, k_stride_h;
    int64_t v_stride_b, v_stride_s, v_stride_h;
    const float* k_scale;           /* (B,Sk,H) */
    const float* v_scale;
    int64_t k_scale_stride_b, k_scale_stride_s;
    int64_t v_scale_stride_b, v_scale_stride_s;
    const uint8_t* dense_mask;      /* (B,Sk) u8, nonzero = visible; NULL = all visible */
    int64_t mask_stride_b;
    int32_t B, Sk, H, D;
    float scale;                    /* softmax scale, > 0 */           
    int32_t k_splits;
    float* out_acc;
    float* lse_acc;
} LwmKv8DecodeArgs;
int lwm_attn_decode_kv8(const LwmKv8DecodeArgs* args, void* stream);

/* A BLOCK of Sq queries over that cache (lwm_version() >= 530): chunked prefill, a block appended to a live cache.
 * Key j < Sk is visible to query i iff j <= q_start + i and key_valid[b, j] != 0 (key_valid NULL: all valid) -- the
 * structured mask of lwm_attn_fwd with causal = 1, k_start = 0.  The kernel is lwm_attn_fwd's split-K kernel with the
 * staging replaced: e4m3 bytes and scales are dequantised on their way into LDS (exactly: q * s is a bf16 number), no
 * bf16 copy of the cache exists in memory, and the partials are bit for bit those of lwm_attn_fwd (final_out = 0, the
 * same k_splits >= 2) over a bf16 copy.  Output: normalised partials out_acc [k_splits,B,Sq,H,D] f32 and lse_acc
 * [k_splits,B,H,Sq] f32 (k_splits 0 and 1: one piece), merged by lwm_attn_combine; a row that sees nothing gives
 * (0, -inf); masked rows and rows at or past Sk contribute nothing whatever their bytes and scales hold.  D = 128,
 * Sq >= 1, Sk >= 1, 0 <= k_splits <= 4096; alignment and strides as lwm_attn_decode_kv8; key_valid_stride_b in bytes. */
typedef struct LwmKv8PrefillArgs {
    LwmTensor4 q;                   /* bf16 (B,Sq,H,D) */
    const void* k;                  /* e4m3 bytes (B,Sk,H,D) */
    const void* v;
    int64_t k_stride_b, k_stride_s, k_stride_h;
    int64_t v_stride_b, v_stride_s, v_stride_h;
    const float* k_scale;           /* (B,Sk,H) */
    const float* v_scale;
    int64_t k_scale_stride_b, k_scale_stride_s;
    int64_t v_scale_stride_b, v_scale_stride_s;
    const uint8_t* key_valid;       /* (B,Sk) u8, nonzero = valid; NULL = all valid */
    int64_t key_valid_stride_b;
    int32_t B, Sq, Sk, H, D;
    int64_t q_start;                /* position of query row 0 (= the cache index the block was written at) */
    float scale;                    /* softmax scale, > 0 */
    int32_t k_splits;
    float* out_acc;
    float* lse_acc;
} LwmKv8PrefillArgs;
int lwm_attn_prefill_kv8(const LwmKv8PrefillArgs* args, void* stream);

/* ------------------------------------------------------------------ 4-bit KV cache (lwm_version() >= 570)
 * The cache in the OCP MXFP4 format: e2m1 codes with one e8m0 scale byte per block of 32 elements.  68 bytes per
 * (row, head) against 256 for bf16 and 132 for the 8-bit cache: 0.27 of the bf16 cache's bytes, in memory and per
 * decode step.  Per layer four tensors:
 *   cached_key, cached_value          uint8 (B, max_length, H, 64): two e2m1 codes per byte, element 2i in the low
 *                                     nibble and element 2i+1 in the high nibble; heads of a row contiguous;
 *   key_scale_e8m0, value_scale_e8m0  uint8 (B, max_length, H, 4): one e8m0 byte b per block of 32 consecutive
 *                                     elements of a head, the scale 2^(b - 127).
 * e2m1: the sign in bit 3; the magnitudes 0, 0.5, 1, 1.5, 2, 3, 4, 6 for the codes 0..7.
 * One block (32 bf16 values x): amax = max |x|; s = the smallest power of two with amax / s <= 6, its biased
 * exponent clamped to [1, 254] (s >= 2^-126; byte 255 is never written), s = 1 (byte 127) when amax == 0;
 * q = e2m1(x / s), round to nearest, ties to the even code (x / s is exact in f32 and in range: nothing saturates;
 * -0 keeps its sign).  This is the 8-bit cache's rule with 6 in place of 448, not the OCP "floor(log2 amax) - 2"
 * rule, which saturates.  q * s is exactly representable in bf16, a normal number whenever s >= 2^-125.  Non-finite
 * inputs are not supported.
 *
 * lwm_kv4_cache_write / _at: the arguments of lwm_kv8_cache_write / _at (row_elems = H * 128; cache and scale batch
 * strides in bytes, src strides in bf16 elements); rows of a batch entry are contiguous (H * 64 and H * 4 bytes).
 * src 16-byte aligned, cache and scale 4-byte aligned; otherwise LWM_EINVAL. */
int lwm_kv4_cache_write(void* cache, const void* src, int32_t B, int64_t cache_stride_b,
                        int64_t src_stride_b, int64_t dst_row0, int64_t src_row0, int64_t nrows,
                        int32_t row_elems, void* scale, int64_t scale_stride_b, int32_t H, void* stream);
int lwm_kv4_cache_write_at(void* cache, const void* src, int32_t B, int64_t cache_stride_b,
                           int64_t src_stride_b, const int32_t* dst_row0_dev, int64_t row_offset,
                           int64_t cache_rows, int64_t src_row0, int64_t nrows, int32_t row_elems,
                           void* scale, int64_t scale_stride_b, int32_t H, void* stream);

/* Cached-decode attention (one query per batch row) over that cache: the contract of lwm_attn_decode_kv8.  The
 * visible key range of each (B, Sk) mask row is partitioned over k_splits pieces, one workgroup each; masked keys
 * inside it contribute nothing whatever their nibbles and scale bytes hold (0xFF included); the normalised partials
 * out_acc [k_splits,B,1,H,D] f32 and lse_acc [k_splits,B,H,1] f32 are merged by lwm_attn_combine; a row with nothing
 * visible gives (0, -inf).  The score of a key is the sum over its four blocks of scale_b * (q_b . k_b).
 * D = 128; q, the cache rows (k/v_stride_* in bytes, a head is 64 contiguous bytes) and out_acc 16-byte aligned;
 * scale strides in bytes, the 4 bytes of a head and the H heads of a row contiguous; 0 <= k_splits <= 4096.
 * Anything else is LWM_EINVAL with a message.  Chunked prefill (a block of queries) over this cache is not built. */
typedef struct LwmKv4DecodeArgs {
    LwmTensor4 q;                   /* bf16 (B,1,H,D) */
    const void* k;                  /* nibble bytes (B,Sk,H,D/2) */
    const void* v;
    int64_t k_stride_b, k_stride_s, k_stride_h;
    int64_t v_stride_b, v_stride_s, v_stride_h;
    const void* k_scale;            /* e8m0 bytes (B,Sk,H,4) */
    const void* v_scale;
    int64_t k_scale_stride_b, k_scale_stride_s;
    int64_t v_scale_stride_b, v_scale_stride_s;
    const uint8_t* dense_mask;      /* (B,Sk) u8, nonzero = visible; NULL = all visible */
    int64_t mask_stride_b;
    int32_t B, Sk, H, D;
    float scale;                    /* softmax scale, > 0 */
    int32_t k_splits;
    float* out_acc;
    float* lse_acc;
} LwmKv4DecodeArgs;
int lwm_attn_decode_kv4(const LwmKv4DecodeArgs* args, void* stream);

/* ------------------------------------------------------------------ 6-bit KV cache (lwm_version() >= 630)
 * The cache in the OCP MXFP6 format: e2m3 codes with one e8m0 scale byte per block of 32 elements.  100 bytes per
 * (row, head) against 256 for bf16, 132 for the 8-bit cache and 68 for the 4-bit one: 0.39 of the bf16 cache's bytes,
 * in memory and per decode step.  Per layer four tensors:
 *   cached_key, cached_value          uint8 (B, max_length, H, 96): head element d belongs to block d / 32; a block is
 *                                     24 bytes and a head row its four blocks in order; element j of a block occupies
 *                                     bits [6j, 6j + 6) of the block's 24 bytes read as one little-endian 192-bit
 *                                     integer (the order in which v_cvt_scalef32_pk32_f32_fp6 reads its six registers);
 *                                     heads of a row contiguous;
 *   key_scale_e8m0, value_scale_e8m0  uint8 (B, max_length, H, 4): as in the 4-bit cache, one e8m0 byte b per block,
 *                                     the scale 2^(b - 127).  (The two caches differ in the last dimension of
 *                                     cached_key: 96 here, 64 there.)
 * e2m3: the sign in bit 5, the exponent (bias 1) in bits 4-3, the mantissa in bits 2-0.  For the magnitude code
 * c = 0..31: c / 8 where c < 8, else (1 + (c & 7) / 8) * 2^((c >> 3) - 1); the largest magnitude is 7.5.  Magnitudes
 * are monotone in c and the mantissa's last bit is the code's last bit, so IEEE round-to-nearest-even is "ties to the
 * even code".
 * One block (32 bf16 values x): amax = max |x|; s = the smallest power of two with amax / s <= 7.5, its biased
 * exponent clamped to [1, 254] (s >= 2^-126; byte 255 is never written), s = 1 (byte 127) when amax == 0;
 * q = e2m3(x / s), round to nearest, ties to the even code (x / s is exact in f32 and in range: nothing saturates;
 * -0 keeps its sign).  This is the 4-bit cache's rule with 7.5 in place of 6.  q * s has at most 4 significant bits:
 * it is exactly representable in bf16, a normal number whenever s >= 2^-123.  Non-finite inputs are not supported, nor
 * is a block whose amax reaches 1.9375 * 2^127 (about 3.30e38): its largest element rounds up to 2^128, past the top of
 * bf16.  Away from the lower clamp: |x - q s| <= s / 4 and s < amax / 3.75, hence |x - q s| < amax / 15;
 * |x - q s| <= 2^-4 |x| for |x| >= s; and element by element the error is never larger than the 4-bit cache's on the
 * same block.
 *
 * lwm_kv6_cache_write / _at: the arguments of lwm_kv4_cache_write / _at (row_elems = H * 128; cache and scale batch
 * strides in bytes, src strides in bf16 elements); rows of a batch entry are contiguous (H * 96 and H * 4 bytes).
 * src 16-byte aligned, cache 8-byte aligned, scale 4-byte aligned; otherwise LWM_EINVAL. */
int lwm_kv6_cache_write(void* cache, const void* src, int32_t B, int64_t cache_stride_b,
                        int64_t src_stride_b, int64_t dst_row0, int64_t src_row0, int64_t nrows,
                        int32_t row_elems, void* scale, int64_t scale_stride_b, int32_t H, void* stream);
int lwm_kv6_cache_write_at(void* cache, const void* src, int32_t B, int64_t cache_stride_b,
                           int64_t src_stride_b, const int32_t* dst_row0_dev, int64_t row_offset,
                           int64_t cache_rows, int64_t src_row0, int64_t nrows, int32_t row_elems,
                           void* scale, int64_t scale_stride_b, int32_t H, void* stream);

/* Cached-decode attention (one query per batch row) over that cache: the contract of lwm_attn_decode_kv4 (masked keys
 * contribute nothing whatever their bytes and scale bytes hold; a row with nothing visible gives (0, -inf); the score of
 * a key is the sum over its four blocks of scale_b * (q_b . k_b)).  D = 128; q and out_acc 16-byte aligned; the cache
 * rows (k/v_stride_* in bytes, a head is 96 contiguous bytes) 8-byte aligned, pointers and strides; scale strides in
 * bytes, the 4 bytes of a head and the H heads of a row contiguous; 0 <= k_splits <= 4096.  Anything else is LWM_EINVAL
 * with a message. */
typedef struct LwmKv6DecodeArgs {
    LwmTensor4 q;                   /* bf16 (B,1,H,D) */
    const void* k;                  /* e2m3 blocks (B,Sk,H,96) */
    const void* v;
    int64_t k_stride_b, k_stride_s, k_stride_h;
    int64_t v_stride_b, v_stride_s, v_stride_h;
    const void* k_scale;            /* e8m0 bytes (B,Sk,H,4) */
    const void* v_scale;
    int64_t k_scale_stride_b, k_scale_stride_s;
    int64_t v_scale_stride_b, v_scale_stride_s;
    const uint8_t* dense_mask;      /* (B,Sk) u8, nonzero = visible; NULL = all visible */
    int64_t mask_stride_b;
    int32_t B, Sk, H, D;
    float scale;                    /* softmax scale, > 0 */
    int32_t k_splits;
    float* out_acc;
    float* lse_acc;
} LwmKv6DecodeArgs;
int lwm_attn_decode_kv6(const LwmKv6DecodeArgs* args, void* stream);

/* A BLOCK of Sq queries over that cache: the contract of lwm_attn_prefill_kv8 (key j < Sk visible to query i iff
 * j <= q_start + i and key_valid[b, j] != 0; lwm_attn_fwd's split-K kernel with the staging replaced; the partials bit
 * for bit those of lwm_attn_fwd with final_out = 0 and the same k_splits >= 2 over a bf16 copy of the dequantised cache;
 * masked rows and rows at or past Sk contribute nothing whatever their bytes and scale bytes hold).  D = 128, Sq >= 1,
 * Sk >= 1, 0 <= k_splits <= 4096; alignment and strides as lwm_attn_decode_kv6; key_valid_stride_b in bytes. */
typedef struct LwmKv6PrefillArgs {
    LwmTensor4 q;                   /* bf16 (B,Sq,H,D) */
    const void* k;                  /* e2m3 blocks (B,Sk,H,96) */
    const void* v;
    int64_t k_stride_b, k_stride_s, k_stride_h;
    int64_t v_stride_b, v_stride_s, v_stride_h;
    const void* k_scale;            /* e8m0 bytes (B,Sk,H,4) */
    const void* v_scale;
    int64_t k_scale_stride_b, k_scale_stride_s;
    int64_t v_scale_stride_b, v_scale_stride_s;
    const uint8_t* key_valid;       /* (B,Sk) u8, nonzero = valid; NULL = all valid */
    int64_t key_valid_stride_b;
    int32_t B, Sq, Sk, H, D;
    int64_t q_start;                /* position of query row 0 (= the cache index the block was written at) */
    float scale;                    /* softmax scale, > 0 */
    int32_t k_splits;
    float* out_acc;
    float* lse_acc;
} LwmKv6PrefillArgs;
int lwm_attn_prefill_kv6(const LwmKv6PrefillArgs* args, void* stream);

/* Elementwise helpers of the ring driver (HBM-bound). */
/* dst_bf16[n] = (bf16) src_f32[n] */
int lwm_cast_f32_to_bf16(const float* src, void* dst, int64_t n, void* stream);
/* dst_bf16[n] = (bf16) (((srcs[0] + srcs[1]) + srcs[2]) + ...), f32 adds in argument order.
 * `srcs` is a HOST array of n_src (1..16) device pointers.  Replaces the f32 dk/dv carry
 * that the reference's backward scan ppermutes around the ring:
 * under the mesh schedule every rank returns its partial straight to the block's owner,
 * which reduces them here. */
int lwm_sum_f32_to_bf16(const float* const* srcs, int32_t n_src, void* dst, int64_t n, void* stream);

/* ------------------------------------------------------------------ RoPE, RMSNorm
 * The HBM-bound steps either side of the attention op. */

/* apply_rotary_emb (lwm/llama.py:353-375): y = x rotated, interleaved (even, odd) pairs as
 * complex numbers times (cos, sin)[pos[b,s]][i]; f32 math, bf16 in/out; y may alias x.
 * table: [max_pos][D/2][2] f32 built on the host as precompute_freqs_cis does
 * (lwm/llama.py:344-350).  conj != 0 rotates by the negative angle (= backward). */
int lwm_rope_bf16(LwmTensor4 x, LwmTensor4 y, const float* table, const int32_t* pos, int32_t B,
                  int32_t S, int32_t H, int32_t D, int32_t max_pos, int32_t conj, void* stream);

/* RMSNorm (lwm/llama.py:320-341) over rows of C bf16: y = bf16(bf16(x * rsqrt(mean(x^2)+eps)) * w).
 * rstd [rows] f32 is written if non-NULL (needed by the backward). */
int lwm_rmsnorm_fwd_bf16(const void* x, const void* w, void* y, float* rstd, int64_t rows, int32_t C,
                         float eps, void* stream);
/* dx [rows,C] bf16 and dw [C] bf16 from g = dL/dy; workspace of
 * lwm_rmsnorm_bwd_workspace_bytes() bytes (f32 partial dW per workgroup). */
int64_t lwm_rmsnorm_bwd_workspace_bytes(int64_t rows, int32_t C);
int lwm_rmsnorm_bwd_bf16(const void* x, const void* w, const void* g, const float* rstd, void* dx,
                         void* dw, void* workspace, int64_t rows, int32_t C, void* stream);
/* The same with the gradient of the residual branch that by-passes the norm folded in (FlaxLLaMABlock,
 * lwm/llama.py:704-744: `x` feeds the norm AND the residual add behind it): dx = bf16(bf16(dx_norm) + res) -- the
 * roundings of a separate bf16 add, one pass less over (rows, C).  res == NULL: lwm_rmsnorm_bwd_bf16. */
int lwm_rmsnorm_bwd_res_bf16(const void* x, const void* w, const void* g, const float* rstd, const void* res,
                             void* dx, void* dw, void* workspace, int64_t rows, int32_t C, void* stream);

/* The SwiGLU gate of FlaxLLaMAMLP (lwm/llama.py:659): y = silu(a) * b and its backward
 * (da, db from g = dL/dy); bf16, n % 8 == 0, all pointers 16-byte aligned. */
int lwm_swiglu_fwd_bf16(const void* a, const void* b, void* y, int64_t n, void* stream);
int lwm_swiglu_bwd_bf16(const void* a, const void* b, const void* g, void* da, void* db, int64_t n,
                        void* stream);
/* The same on (rows, cols) windows of wider buffers (leading dimensions in elements, multiples of 8): gate and up as the
 * two halves of ONE (rows, 2F) GEMM output -- w1 | w3 run as one library GEMM (lwm/llama.py:631-655 share their input) --
 * and d gate | d up written into the halves of the one buffer the fused dgrad / wgrad GEMMs read. */
int lwm_swiglu_fwd_ld_bf16(const void* a, int64_t lda, const void* b, int64_t ldb, void* y, int64_t ldy, int64_t rows,
                           int64_t cols, void* stream);
int lwm_swiglu_bwd_ld_bf16(const void* a, int64_t lda, const void* b, int64_t ldb, const void* g, int64_t ldg, void* da,
                           int64_t ldda, void* db, int64_t lddb, int64_t rows, int64_t cols, void* stream);

/* dst[c][r] = src[r][c], bf16, rows and cols multiples of 64 (leading dimensions in elements).  Serves the library GEMMs
 * around the hot path: flax Dense kernels are (in, out) (lwm/llama.py:390-421, :631-655); hipBLASLt runs fastest with the
 * reduction dimension contiguous in both operands, so the harness re-lays each kernel as (out, in) once per step and
 * transposes the narrow operand of each weight gradient.  HBM-bound (2 x rows x cols x 2 bytes). */
int lwm_transpose_bf16(const void* src, int64_t ld_src, void* dst, int64_t ld_dst, int64_t rows, int64_t cols,
                       void* stream);

/* The weight gradient of a flax Dense kernel (lwm/llama.py:390-421, :631-655: y = x @ W with W (in, out)):
 * dw[K][N] = sum over s of x[s][K] * g[s][N], bf16 operands with the feature dimension contiguous (leading dimensions in
 * elements), f32 accumulation in a fixed order, bf16 result.  S % 32 == 0, K % 256 == 0, N % 256 == 0.  Both operands are
 * read where they lie (no transposed copies): LDS-DMA tiles, transposed MFMA fragments.  Tiles beyond the last whole round
 * of one tile per CU are cut along S (stream-K) and summed from f32 partials in `workspace`
 * (lwm_wgrad_workspace_bytes(S, K, N), 16-byte aligned; may be null when that is 0).
 * FLOPs 2 S K N; HBM bytes 2 (S K + S N + K N) algorithmic. */
int64_t lwm_wgrad_workspace_bytes(int64_t S, int64_t K, int64_t N);
int lwm_wgrad_bf16(const void* x, int64_t ldx, const void* g, int64_t ldg, void* dw, int64_t lddw, int64_t S, int64_t K,
                   int64_t N, void* workspace, int64_t workspace_bytes, void* stream);

/* y[r, :] = x[r, :] . W for rows <= 4 -- the projections of a cached-decode step (one token per batch row
 * against the [K, N] bf16 kernels wq/wk/wv/wo, w1/w2/w3, lm_head; x @ kernel as flax nn.Dense computes it,
 * lwm/llama.py:427-432, :659, :1075-1106).  HBM-bound: W is read once (2*K*N bytes), f32 accumulation in a fixed
 * order (deterministic).  x: [rows, K] bf16, row stride ldx; w: [K, N] bf16 dense; y: [rows, N] bf16 (row
 * stride ldy) and / or y_f32: [rows, N] f32 dense; workspace: lwm_gemv_workspace_bytes() bytes, 16-byte aligned.
 * N % 8 == 0, K % 32 == 0, K <= 12288.
 * lwm_gemv_multi_bf16: 1..3 kernels that share x (wq | wk | wv; w1 | w3) in ONE pair of launches; w, y, ldy,
 * y_f32, N are arrays of nmat entries (y or y_f32 may be NULL as a whole or per entry); workspace: the sum of
 * lwm_gemv_workspace_bytes(rows, K, N[i]). */
int64_t lwm_gemv_workspace_bytes(int32_t rows, int32_t K, int32_t N);
int lwm_gemv_bf16(const void* x, int64_t ldx, const void* w, void* y, int64_t ldy, float* y_f32, void* workspace,
                  int32_t rows, int32_t K, int32_t N, void* stream);
int lwm_gemv_multi_bf16(const void* x, int64_t ldx, int32_t nmat, const void* const* w, void* const* y, const int64_t* ldy,
                        float* const* y_f32, const int32_t* N, void* workspace, int32_t rows, int32_t K, void* stream);

/* The same launch pair with the small launches either side of a decode-step projection riding along (every field but
 * the first block optional, zero = off):
 *   RMSNorm on load  (lwm/llama.py:320-341 in front of wq|wk|wv, w1|w3, lm_head): x is normalised as it is read,
 *     bf16(bf16(x * rstd) * norm_weight[k]) with rstd = 1/sqrt(sum(ss_in[r][0..ss_n)) / K + eps) -- ss_in are partial
 *     sums of squares of x's rows, e.g. the ss_out of the launch that produced x (or one total and zeros);
 *   residual add     (lwm/llama.py:719, :737 behind wo, w2): y = bf16(bf16(x . W) + residual), and
 *   ss_out           [rows][N/128] partial sums of squares of y's rows (one matrix, N % 128 == 0) for the next norm.
 * Results equal the separate launches' (same roundings); rstd may differ in its last bit (other summation order). */
typedef struct LwmGemvArgs {
    const void* x; int64_t ldx; int32_t nmat; int32_t rows, K;
    const void* w[3]; void* y[3]; int64_t ldy[3]; float* y_f32[3]; int32_t N[3];
    void* workspace;
    const void* norm_weight; const float* ss_in; int32_t ss_n; float eps;
    const void* residual[3]; int64_t ldres[3];
    float* ss_out;
} LwmGemvArgs;
int lwm_gemv_fused_bf16(const LwmGemvArgs* args, void* stream);

/* ------------------------------------------------------------------ 8-bit decode weights (lwm_version() >= 550)
 * The projections of a cached-decode step stream every weight once per token; an 8-bit copy of a kernel is 0.516 of the
 * bytes.  A bf16 kernel W of shape [K, N], row-major as the GEMV reads it, becomes
 *   q      uint8 [K, N]               OCP e4m3fn bit patterns (1 sign, 4 exponent bits with bias 7, 3 mantissa bits;
 *                                     exponent 0 = subnormal m * 2^-9; 0x7f / 0xff = NaN), the same layout;
 *   scale  f32   [ceil(K/128), N]     one scale per group of 128 rows of K and per column -- the group is the K tile of
 *                                     one GEMV partial sum.
 * Quantising one group of one column: amax = max |w| over the group's rows that exist (the last group of a K that is
 * no multiple of 128 is shorter); s = the smallest power of two with amax / s <= 448, clamped to [2^-126, 2^127], and
 * s = 1 when amax == 0; q = e4m3(w / s), round to nearest even.  w / s is exact and |w / s| <= 448: nothing saturates,
 * and the bytes 0x7f / 0xff are never written.  Non-finite weights (Inf, NaN) are NOT supported: their group's scale and
 * bytes are unspecified.  The GEMV does not sanitise NaN bytes: they propagate.
 * lwm_w8_quantise: one pass over w [K, N] bf16 -> q, scale and `rounded` [K, N] bf16 = bf16(e4m3(q) * s), the value
 *   the bytes stand for (`rounded` may be w itself: rounding in place).  K % 32 == 0, K <= 12288, N % 8 == 0; every
 *   pointer 16-byte aligned.  No atomics: the same input gives the same bits.
 * lwm_gemv_fused_w8: lwm_gemv_fused_bf16 with w[i] = the bytes and w_scale[i] = the scales of kernel i; every other
 *   field means what it means in LwmGemvArgs (rows <= 4, K % 32 == 0, K <= 12288; N[i] % 8 == 0; workspace of the sum
 *   of lwm_gemv_workspace_bytes(rows, K, N[i]) bytes).  Same K partition, same order of every sum as the bf16 entry; the
 *   scale multiplies each partial sum once.  Exactness domain: e4m3(q) * s has 4 significant bits and is a bf16 value
 *   whenever it is a normal number, and with power-of-two scales and neither overflow nor underflow in the partial sums
 *   (scales between 2^-40 and 2^40 and activations of ordinary size are well inside) the results -- outputs and workspace
 *   partials -- are BIT FOR BIT those of lwm_gemv_fused_bf16 on the `rounded` weights. */
int lwm_w8_quantise(const void* w, void* q, float* scale, void* rounded, int32_t K, int32_t N, void* stream);
typedef struct LwmGemvW8Args {
    const void* x; int64_t ldx; int32_t nmat; int32_t rows, K;
    const void* w[3]; const float* w_scale[3]; void* y[3]; int64_t ldy[3]; float* y_f32[3]; int32_t N[3];
    void* workspace;
    const void* norm_weight; const float* ss_in; int32_t ss_n; float eps;
    const void* residual[3]; int64_t ldres[3];
    float* ss_out;
} LwmGemvW8Args;
int lwm_gemv_fused_w8(const LwmGemvW8Args* args, void* stream);

/* ------------------------------------------------------------------ 4-bit decode weights (lwm_version() >= 580)
 * OCP MXFP4 copies of the same kernels: 4.25 bits per weight, 0.266 of the bf16 bytes and 0.515 of the 8-bit pack's.  A
 * bf16 kernel W of shape [K, N] (K % 32 == 0, K <= 12288, N % 8 == 0) becomes
 *   q      uint8 [K/4][N/8][16]       e2m1 codes (sign in bit 3; magnitudes 0, 0.5, 1, 1.5, 2, 3, 4, 6 for the codes 0..7),
 *                                     two per byte, K * N / 2 bytes.  NOT row-major: slot [k4][n8] holds rows
 *                                     4 k4 .. 4 k4 + 3 of columns 8 n8 .. 8 n8 + 7; byte 4 j + b of the slot holds row
 *                                     4 k4 + j, column 8 n8 + 2 b in its low nibble and column 8 n8 + 2 b + 1 in its high
 *                                     nibble (the nibble order of the 4-bit KV cache).  W[k][n] is therefore the nibble
 *                                     (n & 1) of byte ((k >> 2) * (N / 8) + (n >> 3)) * 16 + (k & 3) * 4 + ((n & 7) >> 1).
 *                                     One 16-byte load of a GEMV lane brings four rows of its eight columns, and the 64
 *                                     lanes of a wave read 1 KiB contiguous;
 *   scale  uint8 [K/32][N]            one e8m0 byte b per MX block -- 32 consecutive rows of K of one column, the rows one
 *                                     wave of the GEMV walks: the scale 2^(b - 127).
 * Quantising one block: the rule of the 4-bit KV cache, not the saturating OCP one.  amax = max |w| over the block; s = the
 * smallest power of two with amax / s <= 6, its exponent byte clamped to [1, 254], and byte 127 when amax == 0;
 * q = e2m1(w / s), round to nearest, ties to the even code.  w / s is exact and |w / s| <= 6: nothing saturates; -0 keeps
 * its sign.  Non-finite weights (Inf, NaN) are NOT supported, nor is a block whose amax exceeds 3.5 * 2^126.
 * lwm_w4_quantise: one pass over w [K, N] bf16 -> q, scale_e8m0 and `rounded` [K, N] bf16 = bf16(e2m1(q) * s), the value
 *   the codes stand for (`rounded` may be w itself: rounding in place).  Every pointer 16-byte aligned.  No atomics: the
 *   same input gives the same bits.
 * lwm_gemv_fused_w4: lwm_gemv_fused_bf16 with w[i] = the codes and w_scale[i] = the scale bytes of kernel i; every other
 *   field means what it means in LwmGemvArgs (rows <= 4, K % 32 == 0, K <= 12288; N[i] % 8 == 0; workspace of the sum of
 *   lwm_gemv_workspace_bytes(rows, K, N[i]) bytes), and the refusals are those of lwm_gemv_fused_w8.  Same K partition,
 *   same order of every sum as the bf16 entry; the block's scale multiplies the sum over the block's 32 rows once.
 *   Exactness domain: e2m1(q) * s has 2 significant bits and is a bf16 value whenever it is a normal number, and with
 *   power-of-two scales and neither overflow nor underflow in the partial sums (scales between 2^-40 and 2^40 and
 *   activations of ordinary size are well inside) the results -- outputs and workspace partials -- are BIT FOR BIT those
 *   of lwm_gemv_fused_bf16 on the `rounded` weights. */
int lwm_w4_quantise(const void* w, void* q, void* scale_e8m0, void* rounded, int32_t K, int32_t N, void* stream);
typedef struct LwmGemvW4Args {
    const void* x; int64_t ldx; int32_t nmat; int32_t rows, K;
    const void* w[3]; const uint8_t* w_scale[3]; void* y[3]; int64_t ldy[3]; float* y_f32[3]; int32_t N[3];
    void* workspace;
    const void* norm_weight; const float* ss_in; int32_t ss_n; float eps;
    const void* residual[3]; int64_t ldres[3];
    float* ss_out;
} LwmGemvW4Args;
int lwm_gemv_fused_w4(const LwmGemvW4Args* args, void* stream);

/* ------------------------------------------------------------------ 6-bit decode weights (lwm_version() >= 640)
 * OCP MXFP6 (e2m3) copies of the same kernels, between the two above: 6.25 bits per weight, 0.391 of the bf16 bytes and
 * 0.757 of the 8-bit pack's, with e4m3's three mantissa bits.  A bf16 kernel W of shape [K, N] (K % 32 == 0, K <= 12288,
 * N % 8 == 0) becomes
 *   q      uint8 [K/4][N/8][24]       e2m3 codes (sign in bit 5, exponent with bias 1 in bits 4-3, mantissa in bits 2-0:
 *                                     magnitude code c = 0..31 is c / 8 below 8 and (1 + (c & 7) / 8) * 2^((c >> 3) - 1) from
 *                                     8 on, 7.5 at most), 3 K N / 4 bytes.  NOT row-major: slot [k4][n8] holds rows
 *                                     4 k4 .. 4 k4 + 3 of columns 8 n8 .. 8 n8 + 7 as 32 codes, code 8 j + c being row
 *                                     4 k4 + j, column 8 n8 + c; code i sits at bits [6 i, 6 i + 6) of the slot's 24 bytes
 *                                     read as one little-endian 192-bit integer (the block convention of the 6-bit KV
 *                                     cache).  W[k][n] is therefore code i = 8 (k & 3) + (n & 7) of the slot at byte
 *                                     ((k >> 2) * (N / 8) + (n >> 3)) * 24.  A slot is 8-byte aligned, not 16-byte aligned;
 *                                     one slot of a GEMV lane brings four rows of its eight columns, and the 64 lanes of a
 *                                     wave read 1536 contiguous bytes;
 *   scale  uint8 [K/32][N]            one e8m0 byte b per MX block -- 32 consecutive rows of K of one column, the rows one
 *                                     wave of the GEMV walks: the scale 2^(b - 127).
 * Quantising one block: the rule of the 4-bit weights with 7.5 in place of 6 (that of the 6-bit KV cache).  amax = max |w|
 * over the block; s = the smallest power of two with amax / s <= 7.5, its exponent byte clamped to [1, 254], and byte 127
 * when amax == 0; q = e2m3(w / s), round to nearest, ties to the even code.  w / s is exact and |w / s| <= 7.5: nothing
 * saturates; -0 keeps its sign.  Non-finite weights (Inf, NaN) are NOT supported, nor is a block whose amax reaches
 * 1.9375 * 2^127 (its largest element would round up to 2^128, past the top of bf16).
 * lwm_w6_quantise: one pass over w [K, N] bf16 -> q, scale_e8m0 and `rounded` [K, N] bf16 = bf16(e2m3(q) * s), the value
 *   the codes stand for (`rounded` may be w itself: rounding in place).  Every pointer 16-byte aligned.  No atomics: the
 *   same input gives the same bits.
 * lwm_gemv_fused_w6: lwm_gemv_fused_bf16 with w[i] = the codes and w_scale[i] = the scale bytes of kernel i; every other
 *   field means what it means in LwmGemvArgs (rows <= 4, K % 32 == 0, K <= 12288; N[i] % 8 == 0; workspace of the sum of
 *   lwm_gemv_workspace_bytes(rows, K, N[i]) bytes), and the refusals are those of lwm_gemv_fused_w8 and lwm_gemv_fused_w4.
 *   Same K partition, same order of every sum as the bf16 entry; the block's scale multiplies the sum over the block's 32
 *   rows once.
 * lwm_gemm_rows_fused_w6 (declared with the other 1..32-row entries below): lwm_gemm_rows_fused_bf16 over the same packs,
 *   the codes becoming the rounded bf16 values e2m3(q) * s on their way to the matrix instruction; refusals as
 *   lwm_gemm_rows_fused_w8.
 * Exactness domain: e2m3(q) * s has 4 significant bits and is a bf16 value whenever it is a normal number, and with
 *   power-of-two scales and neither overflow nor underflow in the partial sums (scales between 2^-40 and 2^40 and
 *   activations of ordinary size are well inside) the results -- outputs and workspace partials -- are BIT FOR BIT those
 *   of lwm_gemv_fused_bf16 (lwm_gemm_rows_fused_bf16 for the rows entry) on the `rounded` weights. */
int lwm_w6_quantise(const void* w, void* q, void* scale_e8m0, void* rounded, int32_t K, int32_t N, void* stream);
typedef struct LwmGemvW6Args {
    const void* x; int64_t ldx; int32_t nmat; int32_t rows, K;
    const void* w[3]; const uint8_t* w_scale[3]; void* y[3]; int64_t ldy[3]; float* y_f32[3]; int32_t N[3];
    void* workspace;
    const void* norm_weight; const float* ss_in; int32_t ss_n; float eps;
    const void* residual[3]; int64_t ldres[3];
    float* ss_out;
} LwmGemvW6Args;
int lwm_gemv_fused_w6(const LwmGemvW6Args* args, void* stream);

/* ------------------------------------------------------------------ decode projections for 1..32 rows (lwm_version() >= 560)
 * The same products on the matrix pipe (v_mfma_f32_16x16x32_bf16) for batches past the GEMV's four rows: W is still read
 * once.  Every field of LwmGemvArgs / LwmGemvW8Args means what it means for lwm_gemv_fused_bf16 / lwm_gemv_fused_w8, with
 *   1 <= rows <= 32 (rows == 0 is refused); K % 32 == 0, K <= 12288; N[i] % 8 == 0; 1..3 matrices that share x;
 *   x 16-byte aligned with ldx % 8 == 0 and norm_weight 16-byte aligned (both are read 16 bytes at a time);
 *   residual and ss_out with ONE matrix only;
 *   workspace of the sum of lwm_gemm_rows_workspace_bytes(rows, K, N[i]) bytes, 16-byte aligned.
 * Refusals return LWM_EINVAL / LWM_EUNSUPPORTED, leave a message in lwm_last_error() and write nothing.
 * Summation contract: K is cut into groups of 128 rows (the GEMV's partition, = the scale groups of the 8-bit format); the
 *   workspace receives one f32 partial per group, [ceil(K/128)][rows][N[i]] per matrix, each accumulated in f32 by the
 *   matrix instruction over exact bf16 x bf16 products, and the partials of an output are added along the GEMV's fixed
 *   tree by the GEMV's reduction (residual add bf16(bf16(x . W) + residual), ss_out, bf16 / f32 stores: the same code).  No
 *   atomics: the same input gives the same bits.  Within a group the order of the sum is the instruction's, so results
 *   agree with lwm_gemv_fused_bf16 to f32 rounding (|y_f32 - exact| <= K 2^-23 sum_k |x_k W_kn|), and bit for bit wherever
 *   every partial sum is exact (small integers).  RMSNorm on load feeds the instruction bit for bit the normalised x the
 *   GEMV feeds its FMAs (the same expression, the same tree over ss_in).
 * Exactness domain of the 8-bit entry: as for lwm_gemv_fused_w8 -- e4m3(q) * s is a bf16 value whenever it is a normal
 *   number, and with power-of-two scales and neither overflow nor underflow in the partial sums (scales between 2^-40 and
 *   2^40 and activations of ordinary size are well inside) outputs and workspace partials are BIT FOR BIT those of
 *   lwm_gemm_rows_fused_bf16 on the `rounded` weights: the bytes become bf16 before the instruction sees them and the
 *   scale multiplies each partial once.
 * Row independence: the bits of output row r depend on x[r], the weights and the fused operands of row r only -- not on
 *   `rows`, not on the row's position in the call, not on what the other rows hold.  A prompt decodes to the same logits
 *   in a batch of 5 as in a batch of 32. */
int64_t lwm_gemm_rows_workspace_bytes(int32_t rows, int32_t K, int32_t N);
int lwm_gemm_rows_fused_bf16(const LwmGemvArgs* args, void* stream);     /* rows 1..32 */
int lwm_gemm_rows_fused_w8(const LwmGemvW8Args* args, void* stream);
int lwm_gemm_rows_fused_w6(const LwmGemvW6Args* args, void* stream);     /* lwm_version() >= 640 */

/* tux.cross_entropy_loss_and_accuracy as used at lwm/train.py:177-181, :192-201, per row of
 * bf16 logits [rows, V] (V % 8 == 0, V <= 32768): nll[r] = logsumexp(row) - row[target[r]] in
 * f32; correct[r] = (first argmax == target[r]) (may be NULL); and, if dlogits != NULL, the
 * fused gradient dlogits[r] = (softmax(row) - onehot(target[r])) * weight[r] (weight NULL = 1).
 * dlogits may alias logits. */
int lwm_softmax_ce_bf16(const void* logits, const int32_t* target, const float* weight, float* nll,
                        int32_t* correct, void* dlogits, int64_t rows, int32_t V, void* stream);

/* ------------------------------------------------------------------ token sampler (lwm_version() >= 510; top_p: >= 590)
 * One decode step's choice of the next token, per output row b (lwm/vision_llama.py:476-560 _sample_vision;
 * lwm/vision_chat.py:201-213 generate(do_sample=True)), in one launch:
 *   logit   cfg_scale == NULL: row b of `logits`; else rows [0,B) are conditional, [B,2B) unconditional (rows = 2B) and
 *           the logit is u + s*(c - u) with s = cfg_scale[b], three f32 roundings (no fused multiply-add);
 *   greedy  temperature == 0: argmax, lowest index on ties;
 *   filter  0 < top_k < V: keep every entry >= the top_k-th largest of logit / temperature (ties at it all stay);
 *   top-p   0 < top_p < 1 (lwm_version() >= 590; 0 or >= 1: no filter; negative or NaN: LWM_EINVAL), after top-k and
 *           normalised over its survivors K, the order of HF's warpers.  With s_j = logit_j / temperature (f32),
 *           w_j = exp(s_j - max_K s), Z = sum of w over K and M(j) = the sum of w_i over i in K with s_i > s_j (the mass
 *           strictly above j):   entry j stays iff j is in K and M(j) < top_p * Z.
 *           The largest entry always stays (M = 0); entries of equal s stay or go together; a -inf entry never stays
 *           while a finite one exists; greedy ignores top_p as it ignores top_k.  This is FlaxTopPLogitsWarper (cumsum <
 *           top_p rolled by one, min_tokens_to_keep = 1) and torch's TopPLogitsWarper, except that a group of equal
 *           values at the boundary is not split.  A row with a +inf or NaN logit, or without a finite one, has no such
 *           mass: K stays whole.
 *           Arithmetic: the kept set S is a prefix of the descending order with S-(eps) <= S <= S+(eps), S+-(eps) =
 *           {j in K: M(j) < top_p * Z * (1 +- eps)} in exact arithmetic on the f32 s, eps = 2^-20 (9.6e-7).  Derivation:
 *           s_j - max is taken in f64, the f32 exponential of its f32 rounding is corrected by the rounding's remainder
 *           in f64 (second-order term < 2e-11) and the weight is kept as an f32, so it carries the exponential's own
 *           error, 2 f32 ulps = 2^-22 at most, and one rounding, 2^-24: delta = 1.25 * 2^-22; weights of subnormal size
 *           add less than V * 2^-126 in all, against M >= 1 for every entry below the largest; the sums are fixed trees
 *           of f64 additions with chains of at most V / 1024 + 160 links (< 2^-33 relative for any V) and top_p * Z is an
 *           f64 product.  M and Z each move by at most delta, so every entry with M outside top_p * Z * (1 +- 2 * delta),
 *           2 * delta = 0.625 * 2^-20, is decided as in exact arithmetic; eps rounds that up to a power of two.
 *   draw    argmax over the kept entries of logit / temperature + g_j, lowest index on ties (Gumbel-max), with
 *           g = -log(-log(u)), u = ((x >> 9) + 0.5) * 2^-23 and x word (j % 4) of Philox4x32-10 (key = seed, counter =
 *           (j / 4, b, step, 0));
 *   step    *step_dev - step_base (DEVICE int32: a captured graph draws new numbers on every replay), or `step` when
 *           step_dev is NULL;
 *   force   force_period > 0 and (step + 1) % force_period == 0: the token is force_token (lwm/vision_llama.py:549-552);
 *   done    done != NULL (u8 [B]): a row whose done[b] is set emits pad; then done[b] |= (token == eos) (eos < 0: none);
 *   outputs tokens[c*B + b] for c < copies (int64: the next step's input ids, both CFG halves with copies = 2) and / or
 *           seq[b*seq_ld + step] when 0 <= step < seq_cols (int64).
 * The token depends on (logits, cfg, temperature, top_k, top_p, seed, b, step) only.  Any V in [1, 2^30]; logits rows ld >= V
 * apart (elements); pointers 4-byte (logits, cfg_scale, step_dev) / 8-byte (tokens, seq) aligned. */
typedef struct LwmSampleArgs {
    const float* logits;       /* [rows][ld] f32 */
    int64_t ld;
    int32_t rows, V;
    const float* cfg_scale;    /* [rows / 2] f32 or NULL */
    float temperature;
    int32_t top_k;
    uint64_t seed;
    const int32_t* step_dev;   /* or NULL */
    int32_t step_base, step;
    int32_t force_period, force_token;
    uint8_t* done;             /* [B] or NULL */
    int64_t eos, pad;
    int64_t* tokens;           /* [copies][B] or NULL */
    int32_t copies;
    int64_t* seq;              /* [B][seq_ld] or NULL */
    int64_t seq_ld;
    int32_t seq_cols;
    float top_p;               /* lwm_version() >= 590, in what was padding: sizeof is unchanged and 0 = no filter */
} LwmSampleArgs;
int lwm_sample_tokens(const LwmSampleArgs* args, void* stream);

/* ------------------------------------------------------------------ fused AdamW (lwm_version() >= 540)
 * The optimiser phase of a training step over a LIST of tensors, one launch per phase: gradient clipping by the global
 * norm (torch.nn.utils.clip_grad_norm_) and AdamW with decoupled weight decay (torch.optim.AdamW) on f32 master weights
 * and f32 moments, with an optional bf16 working copy of each tensor written in the same pass.  Two tables in DEVICE
 * memory drive it:
 *   tensors  one LwmAdamWTensor per tensor.  Every base is 16-byte aligned.  bias_corr1 = 1 - beta1^t and
 *            sqrt_bias_corr2 = sqrt(1 - beta2^t) are computed by the caller in double from THAT tensor's step count t
 *            (torch counts steps per parameter: one that had no gradient in some step lags behind);
 *   chunks   [n_chunks][2] int32: (tensor, chunk of that tensor).  Chunk k of a tensor is its elements
 *            [k * lwm_adamw_chunk(), (k + 1) * lwm_adamw_chunk()), the last one cut at numel; every chunk of every
 *            tensor is listed once, in any order.  An entry that names no element is skipped.
 * lwm_adamw_grad_norm:  grad_partials[c] = sum of g^2 over chunk c in f64; then one workgroup sums the partials in a
 *            fixed order in f64 and writes norms[0] = (float)sqrt(sum) and the clipping coefficient
 *            norms[1] = min(1, max_norm / (norms[0] + 1e-6f)) in f32 (1 when max_norm <= 0).
 * lwm_adamw_step:  reads the coefficient from norms[1] (no host round trip), then per element, in f32, every
 *            operation rounded on its own:
 *              g = g * coef;  m = m * beta1 + g * (1 - beta1);  v = v * beta2 + (g * g) * (1 - beta2)
 *              den = sqrt(v) / sqrt_bias_corr2 + eps
 *              p = p * (1 - lr * weight_decay)      (tensors with decay != 0)
 *              p = p - (lr / bias_corr1) * (m / den)
 *            stores p, m, v and, where copy_bf16 is given, p rounded to bf16 (nearest even); param_partials[c] = sum of
 *            the NEW p^2 over chunk c in f64, and one workgroup writes norms[2] = the parameter norm after the update.
 *            beta1, beta2, 1 - beta1, 1 - beta2, 1 - lr * weight_decay, lr and eps are rounded to f32 once, from the
 *            doubles below; lr / bias_corr1 is one f32 division per tensor.
 * No floating-point atomics and no order that depends on the launch shape: the same inputs give the same bits.
 * Non-finite gradients are not detected; the arithmetic propagates them. */
typedef struct LwmAdamWTensor {
    float* master;             /* [numel] f32: the parameter */
    const void* grad;          /* [numel] bf16 (grad_bf16 != 0) or f32 */
    float* exp_avg;            /* [numel] f32 */
    float* exp_avg_sq;         /* [numel] f32 */
    void* copy_bf16;           /* [numel] bf16 working copy, or NULL */
    int64_t numel;
    int32_t grad_bf16;
    int32_t decay;             /* != 0: weight decay applies to this tensor */
    float bias_corr1;
    float sqrt_bias_corr2;
} LwmAdamWTensor;

typedef struct LwmAdamWArgs {
    const LwmAdamWTensor* tensors;   /* DEVICE [n_tensors] */
    const int32_t* chunks;           /* DEVICE [n_chunks][2] */
    int32_t n_tensors, n_chunks;
    double lr, beta1, beta2, eps, weight_decay;
    double max_norm;                 /* <= 0: no clipping */
    double* grad_partials;           /* DEVICE f64 workspace of phase A */
    int64_t grad_partials_len;       /* its length in elements, >= n_chunks */
    double* param_partials;          /* DEVICE f64 workspace of phase B */
    int64_t param_partials_len;
    float* norms;                    /* DEVICE [3] f32: gradient norm, clipping coefficient, parameter norm */
} LwmAdamWArgs;
int lwm_adamw_grad_norm(const LwmAdamWArgs* args, void* stream);
int lwm_adamw_step(const LwmAdamWArgs* args, void* stream);
/* elements of one chunk of the chunk table (a constant of the library) */
int lwm_adamw_chunk(void);

/* ------------------------------------------------------------------ dropout (lwm_version() >= 650)
 * Residual and embedding dropout of the training step (lwm/llama.py:423 / :618, :656-660, :998 / :1017) over contiguous
 * [B,S,C] tensors, bf16 or f32, C % 8 == 0, every pointer 16-byte aligned:
 *
 *   lwm_dropout_add_*:  y[b,s,c] = round( res[b,s,c] + (keep ? x[b,s,c] * inv : +0) )        res NULL: round(keep ? x * inv : +0)
 *   lwm_dropout_bwd_*:  y[b,s,c] = round( keep ? x[b,s,c] * inv : +0 )                       x = the gradient of y above,
 *                       y = the gradient of x; `res` is not read -- the gradient of res is the incoming gradient itself.
 *
 *   x * inv is ONE f32 product rounded to f32 and the add ONE f32 addition (never a fused multiply-add); `round` is one
 *   round-to-nearest-even to bf16, and nothing for f32.  A dropped element adds exactly +0.  y may alias x or res.
 *
 * The keep mask is a function of the arguments alone -- nothing is stored, nothing has state -- so the backward, a
 * recompute of the forward and a call on the rows [s0, s1) of a tensor with s_offset = s0 see the bits the whole
 * forward saw.  THE RULE: one Philox4x32-10 call (the generator of the token sampler: the round constants and key
 * schedule of rocRAND's philox4x32_10 engine) serves the 8 channels [8v, 8v + 8) of a row,
 *     key     = (key0, key1)
 *     counter = (c / 8, s_offset + s, b, site)                               (32-bit words; s_offset + S <= 2^32)
 *     h(c)    = 16 bits of output word (c % 8) / 2: its LOW half for even c, its HIGH half for odd c
 *     drop    iff h(c) < thr16
 * with thr16 an integer in [0, 65535] that the CALLER computes as round(p * 65536).  The drop probability is therefore
 * EXACTLY thr16 / 65536, not p: p = 0.1 gives thr16 = 6554 and drops 6554 / 65536 = 0.100006... of the elements.  `inv`
 * is the f32 nearest to 1 / (1 - thr16 / 65536), computed by the caller in f64.  thr16 = 0 drops nothing (with inv = 1:
 * the plain rounded sum); thr16 = 65535 keeps an element with probability 2^-16.  `site` tells the call sites of one step
 * apart (lwm_amd/llama.py: 0 the embedding, 1 + 2 i / 2 + 2 i the attention / MLP output of layer i); (key0, key1) is the
 * caller's (seed, step).  The masks are this library's own stream of i.i.d. bits; they are NOT the bits jax's threefry
 * generator gives the reference for the same seed.
 *
 * LWM_EINVAL, checked in this order: x or y NULL; a negative dimension (or s_offset < 0, s_offset + S > 2^32);
 * C % 8 != 0; a misaligned pointer; thr16 > 65535; inv not finite or < 1.  B, S or C equal to 0: LWM_OK, nothing is
 * launched. */
typedef struct LwmDropoutArgs {
    const void* x;             /* [B,S,C] */
    const void* res;           /* [B,S,C] or NULL */
    void* y;                   /* [B,S,C] */
    int32_t B, S, C;
    int64_t s_offset;          /* the row of the whole sequence that row 0 of these tensors is */
    uint32_t site, key0, key1;
    uint32_t thr16;
    float inv;
} LwmDropoutArgs;
int lwm_dropout_add_bf16(const LwmDropoutArgs* args, void* stream);
int lwm_dropout_add_f32(const LwmDropoutArgs* args, void* stream);
int lwm_dropout_bwd_bf16(const LwmDropoutArgs* args, void* stream);
int lwm_dropout_bwd_f32(const LwmDropoutArgs* args, void* stream);

/* ------------------------------------------------------------------ VQGAN
 * Primitives of the video tokeniser, lwm/vqgan.py.  All tensors are f32, NHWC,
 * dense; results are bit-exact with oracle/vqgan_ref.c (exact-f32 MFMA, fixed
 * summation order -- see DESIGN.md "VQGAN arithmetic contract").
 */

/* flax nn.Conv (kernel HWIO [KH,KW,Cin,Cout], bias) on x [B,Hin,Win,Cin] ->
 * y [B,Ho,Wo,Cout].  Output (oy,ox), tap (kh,kw) reads the virtual input
 * (x upsampled nearest by 2^up_shift) at (oy*stride+kh-pad, ox*stride+kw-pad),
 * zero outside.  Replaces:
 *   3x3 SAME  (stride 1, pad 1)                     lwm/vqgan.py:155,163,172-175,183,253,257
 *   1x1       (stride 1, pad 0)                     lwm/vqgan.py:114-115,262
 *   Downsample (stride 2, pad 0, Ho=Hin/2: the jnp.pad of one zero row/column at
 *              bottom/right is the zero fill)       lwm/vqgan.py:286-303
 *   Upsample  (up_shift 1, stride 1, pad 1)         lwm/vqgan.py:306-319
 * residual (same shape as y, may be NULL) is added after the bias
 * (ResnetBlock, lwm/vqgan.py:263); clip != 0 clamps to [-1,1] (lwm/vqgan.py:141). */
typedef struct LwmConvArgs {
    const float* x;
    const float* w;
    const float* bias;     /* [Cout] or NULL */
    const float* residual; /* [B,Ho,Wo,Cout] or NULL */
    float* y;
    int32_t B, Hin, Win, Cin, Cout, KH, KW, stride, pad, up_shift, Ho, Wo, clip;
} LwmConvArgs;
int lwm_conv2d_nhwc_f32(const LwmConvArgs* args, void* stream);

/* The same convolution in the opt-in second precision (lwm_version() >= 620): operands rounded to bf16 (round to
 * nearest even), products exact, f32 accumulation, on v_mfma_f32_32x32x16_bf16.  NOT bit-exact with the oracle; the
 * contract is |y - y64| <= (K + 2) 2^-23 (sum |bf16(x) bf16(w)| + |bias| + |residual|), K = KH KW Cin, y64 the fp64
 * convolution of the rounded operands, and exact results wherever every partial sum is an integer below 2^24.
 * The struct is the one above with ONE difference: `w` points at the PACKED kernel,
 *     bf16 [KH*KW][Cin/8][Cout][8]:  element (kh, kw, ci, co) at (((kh*KW + kw) * Cin/8 + ci/8) * Cout + co) * 8 + ci%8
 * (a lane's B fragment of the matrix instruction, 8 consecutive input channels of one output channel, is one 16-byte
 * load; lwm_amd.ops.conv_pack_bf16 builds it from the HWIO kernel).  x, bias, residual and y stay f32: x is rounded
 * inside the kernel, on its way into LDS.  Out-of-image taps are exact zeros and are never read; the order of the sum
 * depends on the launch geometry alone: the same call twice gives the same bits, and an image's bits do not depend on
 * the rest of the batch.  Normal numbers only: subnormal and non-finite operands are outside the contract.
 * Cin % 32 == 0 and Cout % 32 == 0 (every VQGAN layer but the two 3-channel ends), otherwise LWM_EUNSUPPORTED;
 * null / misaligned / bad-dimension arguments are refused as by the f32 entry. */
int lwm_conv2d_nhwc_bf16(const LwmConvArgs* args, void* stream);

/* flax nn.GroupNorm (num_groups G, eps, affine) over x [B,HW,C], optionally
 * followed by nn.silu (lwm/vqgan.py:161-162,181-182,251-255).  `workspace` is
 * caller-owned device memory of lwm_groupnorm_workspace_bytes() bytes (f64
 * slice partials, then the f32 mean / rstd per image and group); y may alias x. */
int64_t lwm_groupnorm_workspace_bytes(int32_t B, int64_t HW, int32_t C, int32_t G);
int lwm_groupnorm_silu_f32(const float* x, const float* gamma, const float* beta, float* y,
                           void* workspace, int32_t B, int64_t HW, int32_t C, int32_t G, float eps,
                           int32_t silu, void* stream);

/* VectorQuantizer (lwm/vqgan.py:187-221), D = 64.
 * lwm_vq_sqnorm_f32 : se[e] = |codebook[e]|^2 (once per codebook)
 * lwm_vq_argmin_f32 : idx[n] = first argmin_e (|z_n|^2 + se[e]) - 2 z_n.e   (:207-212)
 * lwm_vq_gather_f32 : out[n] = codebook[idx[n]] (z NULL; decode path :204-205) or the
 *                     forward value of z + stop_gradient(z_q - z) (:214) */
int lwm_vq_sqnorm_f32(const float* codebook, float* se, int32_t E, int32_t D, void* stream);
int lwm_vq_argmin_f32(const float* z, const float* codebook, const float* se, int32_t* idx,
                      int64_t N, int32_t E, int32_t D, void* stream);
int lwm_vq_gather_f32(const float* codebook, const int32_t* idx, const float* z, float* out,
                      int64_t N, int32_t E, int32_t D, void* stream);

/* ------------------------------------------------------------------ frame preprocessor (lwm_version() >= 600)
 * uint8 RGB frames [T,H,W,3] -> f32 [T,size,size,3] in [-1,1]: the resize (Pillow's antialiased bicubic), centre crop
 * and scale of lwm/vision_chat.py:59-74, bit for bit.  Pillow's 8-bit resample is integer arithmetic on fixed-point
 * coefficients; the device does that arithmetic and nothing else, and the CALLER supplies the tables (HOST memory;
 * lwm_amd/frames.py::resample_tables builds them in f64):
 *
 *   a pass (`in` samples -> the `size` samples of the crop window) is, per output sample i,
 *     bounds[i] = {first, taps}                         0 <= first, 1 <= taps <= ksize, first + taps <= in
 *     coeffs[i][0..taps)                                int32, round(weight * 2^22)
 *     result = clamp((2^21 + sum_x pixel[first + x] * coeffs[i][x]) >> 22, 0, 255)     (arithmetic shift; the sum
 *     is taken modulo 2^32: exact while 255 * sum |coeff| + 2^21 < 2^31, which Pillow's tables keep with room to
 *     spare -- tests/test_frames_ref.py)
 *   the horizontal pass (h_*: in = W) runs first and its result is rounded to uint8, as Pillow's intermediate image
 *   is; then the vertical pass (v_*: in = H).  Only the columns and rows of the crop window are tabulated and computed,
 *   and only the rows that the vertical tables read go through the horizontal pass.
 *   ksize 0 (bounds and coeffs NULL) = Pillow skips that pass (output length == input length): the window is COPIED,
 *   from column `left` / row `top` on (otherwise `left` / `top` are ignored).
 *   scale[256] = the f32 value of each byte, float32(u) / float32(127.5) - float32(1).
 *
 * The tables are validated on the host before anything is launched, then copied to the head of `workspace` on
 * `stream`; they must stay valid until the stream has passed this call.  frames, out, workspace are DEVICE memory;
 * workspace: 16-byte aligned, lwm_frames_preprocess_workspace_bytes() bytes (tables + the uint8 intermediate image).
 * LWM_EINVAL: a null pointer, T / H / W / size < 1, a bound pair outside the input, taps > ksize, a window of a
 * skipped pass outside the input, a workspace that is too small or misaligned. */
typedef struct LwmFramesArgs {
    const uint8_t* frames;     /* device [T,H,W,3] */
    float* out;                /* device [T,size,size,3] */
    void* workspace;           /* device */
    int64_t workspace_bytes;
    const int32_t* h_bounds;   /* host [size,2] */
    const int32_t* h_coeffs;   /* host [size,h_ksize] */
    const int32_t* v_bounds;   /* host [size,2] */
    const int32_t* v_coeffs;   /* host [size,v_ksize] */
    const float* scale;        /* host [256] */
    int32_t T, H, W, size, h_ksize, v_ksize, left, top;
} LwmFramesArgs;
int64_t lwm_frames_preprocess_workspace_bytes(int32_t T, int32_t H, int32_t size, int32_t h_ksize, int32_t v_ksize);
int lwm_frames_preprocess_u8(const LwmFramesArgs* args, void* stream);

const char* lwm_last_error(void);
int lwm_version(void);
/* sizeof(LwmAttnArgs) (which = 0) / sizeof(LwmConvArgs) (1) / sizeof(LwmRingArgs) (2) / sizeof(LwmGemvArgs) (3) /
 * sizeof(LwmSampleArgs) (4) / sizeof(LwmKv8DecodeArgs) (5) / sizeof(LwmKv8PrefillArgs) (6) / sizeof(LwmAdamWArgs) (7) as
 * sizeof(LwmAdamWTensor) (8: an element of a device table that the caller lays out) / sizeof(LwmGemvW8Args) (9) /
 * sizeof(LwmKv4DecodeArgs) (10) / sizeof(LwmGemvW4Args) (11) / sizeof(LwmFramesArgs) (12) /
 * sizeof(LwmKv6DecodeArgs) (13) / sizeof(LwmKv6PrefillArgs) (14) / sizeof(LwmGemvW6Args) (15) /
 * sizeof(LwmDropoutArgs) (16) as compiled into the library:
 * lets a foreign-language binding verify its struct mirror at load time. */
int lwm_sizeof(int which);

#ifdef __cplusplus
}
#endif
#endif /* LWM_HIP_H */
