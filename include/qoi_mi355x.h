/*
 * qoi_mi355x.h — C-ABI of libqoi_mi355x.so, the MI355X-native QOI encode/decode path.
 *
 * Part 1 is the DROP-IN boundary: the same four symbols, constants and struct the
 * reference exposes (phoboslab/qoi qoi.h:214-295).  A caller that includes the
 * reference's qoi.h WITHOUT defining QOI_IMPLEMENTATION (prototypes only) and links
 * this library gets the GPU path with no source change; see INTEGRATION.md.
 *
 * Part 2 is ADDITIVE (nothing like it exists in the reference): device-resident
 * batch entry points for callers whose pixels/streams already live in HBM.  Plain
 * pointers and sizes only — no torch / HIP types in any signature (a hipStream_t is
 * passed as void*).
 *
 * All work is done by hand-written gfx950 kernels (the .hip files under qoi_amd/csrc).  There is no
 * CPU fallback: without a usable GPU every entry point fails (NULL / negative status)
 * and qoimi_last_error() says why.
 */
#ifndef QOI_MI355X_H
#define QOI_MI355X_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------
 * Part 1 — drop-in for the reference API
 * ------------------------------------------------------------------------------------ */

#ifndef QOI_H            /* the reference header may already have declared these */
#define QOI_H

#define QOI_SRGB   0     /* qoi.h:233 */
#define QOI_LINEAR 1     /* qoi.h:234 */

/* qoi.h:236-241 — 12 bytes, fields at offsets 0/4/8/9. */
typedef struct {
    unsigned int width;
    unsigned int height;
    unsigned char channels;
    unsigned char colorspace;
} qoi_desc;

/* Replaces qoi.h:278 / implementation qoi.h:356-486.
 * Same contract: NULL on data/desc/out_len == NULL, width or height 0, channels not 3/4,
 * colorspace > 1 or height >= 400000000/width; otherwise a malloc()ed buffer (caller
 * free()s it) holding a stream BYTE-IDENTICAL to the reference encoder's, *out_len set.
 * The buffer holds at least *out_len bytes; the reference's is always the worst-case size
 * (qoi.h:374-379), which nothing in its contract lets a caller rely on. */
void *qoi_encode(const void *data, const qoi_desc *desc, int *out_len);

/* Replaces qoi.h:289 / implementation qoi.h:488-590.
 * Same contract incl. leniency (truncated streams repeat the last pixel, trailer content
 * ignored, over-long runs clipped, ...): result pixels are bit-identical to the
 * reference decoder's for EVERY input stream; desc is filled before validation. */
void *qoi_decode(const void *data, int size, qoi_desc *desc, int channels);

/* Replace qoi.h:252 / qoi.h:595-617 and qoi.h:265 / qoi.h:619-646 (stdio wrappers). */
int   qoi_write(const char *filename, const void *data, const qoi_desc *desc);
void *qoi_read(const char *filename, qoi_desc *desc, int channels);

#endif /* QOI_H */

/* ------------------------------------------------------------------------------------
 * Part 2 — additive device-resident API
 * ------------------------------------------------------------------------------------ */

typedef struct qoimi_ctx qoimi_ctx;

enum {
    QOIMI_OK            =  0,
    QOIMI_E_ARG         = -1,   /* argument rejected by the same rules as qoi.h:364-372 / 497-521 */
    QOIMI_E_NO_GPU      = -2,   /* no usable gfx950 device (none present, wrong architecture, driver missing) */
    QOIMI_E_NOMEM       = -3,
    QOIMI_E_INTERNAL    = -4    /* any other HIP runtime error (e.g. a rejected launch), or a device-side liveness bound tripped */
};

/* Synthetic content classes (qoi_amd/synth.py states the exact per-pixel function). */
enum { QOIMI_NOISE = 0, QOIMI_PHOTO = 1, QOIMI_UIFLAT = 2, QOIMI_CONSTANT = 3, QOIMI_PHOTO_HARD = 4, QOIMI_SPRITE_ALPHA = 5 };

/* Create / destroy a context bound to one GPU.  A context owns a growable device
 * workspace, so steady-state calls do no hipMalloc/hipFree.  ONE call at a time per
 * context: the workspace (scratch, flags, staging) belongs to the call in flight, so a
 * second qoimi_encode_batch / qoimi_decode_batch on the same context must not start -
 * on any stream - before the first one's work has completed (qoimi_decode_batch returns
 * complete; after qoimi_encode_batch synchronise the stream or call qoimi_encode_status).
 * Use one context per thread / per concurrent stream.  The drop-in functions above do
 * exactly that internally: every calling thread gets its own context and stream, so they
 * are re-entrant like the reference (qoi.h:339,357-362,489-495).  Entry points leave the
 * calling thread's current HIP device as they found it. */
int  qoimi_ctx_create(int device, qoimi_ctx **out);
void qoimi_ctx_destroy(qoimi_ctx *ctx);

/* Thread-local description of the last failure in this thread ("" if none). */
const char *qoimi_last_error(void);

/* Worst-case stream size w*h*(channels+1)+14+8 — the reference's allocation, qoi.h:374-376.
 * Returns 0 if desc is rejected. */
size_t qoimi_encode_bound(const qoi_desc *desc);

/* Encode n_images equally-shaped images that live in device memory.
 *   d_pixels       device pointer; image i starts at d_pixels + i*pixel_stride (tightly
 *                  packed row-major w*h*channels bytes, as qoi.h:406-413 reads them)
 *   d_streams      device pointer; stream i is written at d_streams + i*stream_stride,
 *                  stream_stride >= qoimi_encode_bound(desc)
 *   d_stream_len   device int[n_images]; receives each stream's length (= *out_len)
 *   stream         hipStream_t (as void*), NULL = default stream
 * Asynchronous: kernels are enqueued on `stream`; nothing is synchronised. */
int qoimi_encode_batch(qoimi_ctx *ctx, const void *d_pixels, size_t pixel_stride,
                       const qoi_desc *desc, int n_images,
                       void *d_streams, size_t stream_stride, int *d_stream_len,
                       void *stream);

/* The same for images of DIFFERENT shapes and channel counts in one call (a directory of images, qoibench.c:491-555):
 *   pixel_offsets  HOST size_t[n_images]: image i starts at d_pixels + pixel_offsets[i] (tightly packed, as above)
 *   descs          HOST qoi_desc[n_images]: every one must pass the rules of qoi.h:364-372
 *   stream_offsets HOST size_t[n_images]: stream i is written at d_streams + stream_offsets[i]; the caller leaves
 *                  qoimi_encode_bound(&descs[i]) bytes there
 * Streams are byte-identical to the reference encoder's.  Every set of slabs parks its bytes in a scratch slot of its own and two
 * more passes place them (no set waits for another, whatever the mix of sizes): about 5 bytes of workspace per pixel of the call.
 * Enqueues on `stream`; the call itself waits for the stream's earlier work once (its image table travels through pinned staging). */
int qoimi_encode_images(qoimi_ctx *ctx, const void *d_pixels, const size_t *pixel_offsets, const qoi_desc *descs, int n_images,
                        void *d_streams, const size_t *stream_offsets, int *d_stream_len, void *stream);

/* The encoder's colour-table probe uses one LDS exchange instruction per 64 pixels and relies on the LDS serving the lanes of
 * that instruction in ascending order - a MEASURED property of gfx950, not a documented one (qoi_amd/csrc/qoi_encode.hip).  It
 * is measured alone and under contention when a context is created (a failure selects the order-independent probe) and again
 * every 256 encode calls of the context (env QOIMI_ENC_RECHECK_EVERY) on the context's private stream; that repeat is looked at
 * by the NEXT encode call.  Failure latency, stated plainly: if a repeat ever failed, up to 2 x 256 earlier calls of the
 * context would already have returned streams made with the suspect probe.  The context then switches to the order-independent
 * probe for good; the call that notices is encoded with it and returns QOIMI_OK (its own stream is sound), qoimi_last_error()
 * says what happened, the next qoimi_encode_status() returns QOIMI_E_INTERNAL ONCE, and this counter returns how many calls were
 * made since the launch of the last check that passed (the calls before the failed repeat was launched and the ones made while
 * it ran) - re-verify (qoimi_verify_images checks streams against the pixels they were made from, on the device) or re-encode those.  0 = never.
 * QOIMI_ENC_PROBE=0 in the environment selects the order-independent probe from the start (about 1.5 x the encode time). */
long long qoimi_encode_suspect_calls(qoimi_ctx *ctx);

/* Synchronise `stream`.  If a placement wait of the last qoimi_encode_batch on this context gave up (never observed: a set waits for
 * sets that are resident or done - with tickets by construction, for calls of fewer than 8 images by the order the dispatcher starts
 * workgroups in, which launches of other streams could in principle disturb; such waits are bounded and end each other) the call is
 * encoded again here, order-free, from the caller's buffers - which the caller must therefore not have released or overwritten before
 * asking.  QOIMI_E_INTERNAL if that failed too, or - once - after a repeat of the LDS-order self-test failed (see
 * qoimi_encode_suspect_calls); QOIMI_OK otherwise.  A caller that only synchronises its stream never learns of a wait that gave up:
 * call this before reading the streams. */
int qoimi_encode_status(qoimi_ctx *ctx, void *stream);

/* How qoimi_encode_batch hands out the work units of calls of fewer than 8 images (tree placement, where a set waits for the byte
 * counts of lower-numbered sets).  by_workgroup_index = 0 (default): by one ticket per workgroup, i.e. in START order - whatever a set
 * waits for is running or done, on a shared device too; a caller that only synchronises its stream reads complete streams.
 * by_workgroup_index = 1: by workgroup index - 4 us less per 4K frame, correct only as long as the dispatcher starts lower-numbered
 * workgroups no later than higher ones (true of one launch on an idle device); its waits are bounded, a wait that gives up ends the
 * launch's waits and leaves an error flag, and the caller MUST call qoimi_encode_status before reading the streams (it encodes the
 * call again order-free).  The drop-in qoi_encode uses this form and does that by itself.  Returns QOIMI_OK or QOIMI_E_ARG. */
int qoimi_set_encode_small_call_order(qoimi_ctx *ctx, int by_workgroup_index);

/* Calls of this context that qoimi_encode_status encoded again order-free because a placement wait had given up (0: never). */
long long qoimi_encode_retries(qoimi_ctx *ctx);

/* Decode n_images streams that live in device memory.
 *   d_streams      stream i starts at d_streams + i*stream_stride and is sizes[i] bytes
 *   sizes          HOST int[n_images] (the `size` argument of qoi.h:289 per image)
 *   descs          HOST qoi_desc[n_images]: the header of each stream as parsed by the
 *                  caller (what qoi_decode would write to *desc); the images may differ in
 *                  shape - each must decode to w*h*out_channels <= pixel_stride bytes - but
 *                  share the output channel count (channels, or their headers' when it is 0)
 *   channels       0, 3 or 4 — as qoi.h:289
 *   d_pixels       image i is written at d_pixels + i*pixel_stride
 * Synchronous: returns when every pixel is written and verified (the exactness check of the speculative decoder is read
 * before returning).  For calls of a few images the call returns on result words its last launch writes to pinned memory
 * when everything in front of it is done; that launch itself - it writes nothing a caller can see - may still be retiring on
 * `stream` for a few microseconds.  Work the caller enqueues on `stream` is ordered behind it; the context's next call waits
 * for it by itself if it comes on another stream. */
int qoimi_decode_batch(qoimi_ctx *ctx, const void *d_streams, size_t stream_stride,
                       const int *sizes, const qoi_desc *descs, int n_images, int channels,
                       void *d_pixels, size_t pixel_stride, void *stream);

/* The same for streams and images wherever the caller put them - the decoder's counterpart of qoimi_encode_images:
 *   stream_offsets HOST size_t[n_images]: stream i is sizes[i] bytes at d_streams + stream_offsets[i]
 *   pixel_offsets  HOST size_t[n_images]: image i is written tightly packed (w*h*out_channels bytes) at d_pixels + pixel_offsets[i]
 *   sizes, descs, channels: as above; the images may differ in shape and share the output channel count
 * ANY byte offsets, in any order, with gaps or none: streams back to back as qoimi_pack_streams leaves them (align 1 included), images
 * back to back, image 5 in front of image 0.  Exactly w*h*out_channels bytes are written per image and not one byte beside them.  Input
 * ranges may overlap or coincide (one stream decoded twice); OUTPUT ranges must not overlap: QOIMI_E_ARG.  Everything the host can see -
 * sizes[i] < 22, a rejected descriptor, channels, mixed output channel counts, overlapping outputs - is rejected before anything is
 * launched; the caller's buffers are then untouched.  Same rules, same leniency, same synchronous return, same bit-exactness for EVERY
 * input stream as qoimi_decode_batch, which is a caller of the same path (offsets i*stride).
 * Speed: the call is laid out by ascending stream offset internally, so a pack read in any order decodes like a sorted one; a call whose
 * pixel offsets do not ascend with its stream offsets is still exact, but images that lie in front of their neighbours are written with
 * plain stores (slower); so is a stream that ENDS behind the end of the stream that follows it (it takes the full parse, counted in
 * qoimi_decode_stats [3]). */
int qoimi_decode_images(qoimi_ctx *ctx, const void *d_streams, const size_t *stream_offsets, const int *sizes,
                        const qoi_desc *descs, int n_images, int channels,
                        void *d_pixels, const size_t *pixel_offsets, void *stream);

/* Streams back to back, on the device: stream i (d_stream_len[i] bytes at d_streams + i*stream_stride - what qoimi_encode_batch and
 * qoimi_hash_streams take; after qoimi_encode_images a caller that used stream_offsets[i] = i*stride can use it as well) is copied to
 * d_packed + d_packed_off[i].
 *   d_packed_off   DEVICE unsigned long long[n_streams + 1], written by the call: the exclusive scan of the lengths, every start rounded up
 *                  to `align`; d_packed_off[n_streams] is the END of the last stream (not rounded) = the bytes the pack needs
 *   align          a power of two, 1..256 (1: back to back).  Gap bytes between aligned streams are not written.
 *   packed_capacity bytes at d_packed.  A stream that does not fit WHOLLY below it is not copied, not in part; d_packed_off is complete
 *                  in any case, so d_packed_off[n_streams] > packed_capacity says what happened and how much to allocate.  Nothing at or
 *                  behind d_packed + packed_capacity is ever written.  packed_capacity 0 (d_packed may then be NULL): offsets only.
 * Asynchronous on `stream`: no host synchronisation, no read-back - lengths are read and offsets written on the device, so the call can
 * be enqueued straight behind qoimi_encode_batch.  Source [d_streams, + n_streams*stream_stride) and destination [d_packed, +
 * packed_capacity) must not overlap (QOIMI_E_ARG).  stream_stride may be any value (odd too), source and destination any alignment.
 * A length outside [0, stream_stride] is the caller's error; it is clamped to that range, so nothing outside the source range is read -
 * but for the aligned 4-byte words that hold a stream's first and last byte. */
int qoimi_pack_streams(qoimi_ctx *ctx, const void *d_streams, size_t stream_stride, const int *d_stream_len, int n_streams,
                       unsigned align, void *d_packed, size_t packed_capacity,
                       unsigned long long *d_packed_off /* device, n_streams + 1 */, void *stream);

/* Pixels in, pack out, in one call: the result is DEFINED as that of qoimi_encode_batch into a buffer of stride S, qoimi_encode_status, then
 * qoimi_pack_streams(..., align, d_packed, packed_capacity, d_packed_off, ...) over all n_images streams - the same pack bytes, the same
 * d_packed_off[0 .. n_images] (starts rounded up to `align`, [n_images] the unrounded end = the bytes the pack needs), the same d_stream_len -
 * but the caller never owns n_images * S bytes of strided streams: the context encodes consecutive sub-batches of whole images into a staging
 * arena of its own and appends each to the pack on the device (the running end of the pack never travels through the host).
 *   d_packed_off   DEVICE unsigned long long[n_images + 1], d_stream_len DEVICE int[n_images]: written by the call
 *   packed_off_out HOST unsigned long long[n_images + 1], stream_len_out HOST int[n_images], each may be NULL: copies of the two device
 *                  tables, as qoimi_decode_images, qoimi_read_descs and qoimi_inspect_streams take them
 *   align, packed_capacity: as qoimi_pack_streams - a stream that does not fit WHOLLY below packed_capacity is not copied, not in part, gap
 *                  bytes are not written, nothing at or behind d_packed + packed_capacity is written, both tables are complete in any case;
 *                  packed_capacity 0 (d_packed may then be NULL): lengths and offsets only.  An overflow is NOT an error: the call returns
 *                  QOIMI_OK and packed_off_out[n_images] > packed_capacity says what happened and how much to allocate.
 *   staging_bytes  device memory the call may hold for strided streams (an arena of the context, counted in qoimi_workspace_bytes [0], grown
 *                  like the other arenas; a mixed-shape call adds 8 bytes per image for a table).  0: 1 GiB.  The sub-batch plan (normative;
 *                  qoi_amd/packplan.py: plan states it in Python): a slot is qoimi_encode_bound(desc_i) rounded up to 256 bytes, images are
 *                  taken in order, a sub-batch closes when the next slot would not fit in staging_bytes; a request smaller than one slot is
 *                  raised to that slot, so every sub-batch holds at least one image.  Equal shapes: max(1, staging_bytes / slot) images each.
 * Descriptors and pixel_stride are checked by the rules of qoimi_encode_batch; NULL ctx / d_pixels / desc / d_packed_off / d_stream_len,
 * n_images <= 0, align not a power of two in 1..256 and d_packed == NULL with packed_capacity != 0 are rejected as well.  Every rejection
 * (QOIMI_E_ARG) happens before anything is launched: the caller's buffers are untouched.
 * SYNCHRONOUS: returns when the pack, both device tables and the non-NULL host tables are complete.  Every sub-batch is encoded, then its
 * status is looked at exactly as qoimi_encode_status does (a placement wait that gave up is repaired before the sub-batch is copied: the pack
 * never takes bytes from a sub-batch whose status has not been looked at), then it is appended.  A failure of that status (QOIMI_E_INTERNAL,
 * the once-only report of a failed LDS-order repeat included) ends the call with that code; the pack is then incomplete.  Afterwards
 * qoimi_encode_status returns QOIMI_OK and never encodes "the last call" again - it went into staging.
 * Each sub-batch counts as ONE encode call for the counters of the LDS-order self-test (qoimi_encode_suspect_calls, the repeat every 256
 * calls).  d_pixels and [d_packed, + packed_capacity) must not overlap. */
int qoimi_encode_packed(qoimi_ctx *ctx, const void *d_pixels, size_t pixel_stride, const qoi_desc *desc, int n_images,
                        unsigned align, void *d_packed, size_t packed_capacity,
                        unsigned long long *d_packed_off /* device, n_images + 1 */, int *d_stream_len /* device, n_images */,
                        size_t staging_bytes,
                        unsigned long long *packed_off_out /* host, n_images + 1, may be NULL */,
                        int *stream_len_out /* host, n_images, may be NULL */, void *stream);

/* The same for images of different shapes and channel counts, defined the same way with qoimi_encode_images (pixel_offsets, descs: HOST
 * arrays as there; every descriptor is checked before anything is launched). */
int qoimi_encode_images_packed(qoimi_ctx *ctx, const void *d_pixels, const size_t *pixel_offsets, const qoi_desc *descs, int n_images,
                               unsigned align, void *d_packed, size_t packed_capacity,
                               unsigned long long *d_packed_off, int *d_stream_len, size_t staging_bytes,
                               unsigned long long *packed_off_out, int *stream_len_out, void *stream);

/* Tiles and pyramid levels of device images as a pack: the ingest side of the tile server the gather calls below serve.  The caller holds
 * images in device memory, tightly packed as qoimi_encode_images takes them, and names TILES; it never owns a tile's pixels or a strided stream.
 * The result (normative; qoi_amd/tiles.py: tile states it in Python by composing the models of the calls below).  For tile j, S is image
 * tiles[j].image as the caller holds it, sch = descs[image].channels bytes per pixel; R = S[y .. y + height) x [x .. x + width); T is the
 * qoimi_decode_thumbnails reduction of R by `factor` in `mode` at sch channels (with 3 channels QOIMI_THUMB_ALPHA_WEIGHTED is PLAIN, as
 * everywhere), tw = ceil(width / factor) by th = ceil(height / factor) pixels; T is mirrored as qoimi_decode_crops mirrors (QOIMI_CROP_FLIP_X /
 * _Y), then converted to och = channels, or sch when channels is 0 (tiles of 3- and 4-channel images then mix in one call): 4 to 3 drops
 * alpha - after the reduction, so an alpha-weighted reduction keeps its colours -, 3 to 4 sets alpha to 255.  Stream j is the reference
 * encoder's stream, byte for byte, of T with the descriptor {tw, th, och, descs[image].colorspace}.  The pack, d_packed_off[0 .. n_tiles],
 * d_stream_len and the two host tables are exactly what qoimi_encode_images_packed gives over the n_tiles images T in tile order: align, the
 * "a stream that does not fit WHOLLY is not copied, not in part" rule, packed_capacity 0, an overflow returning QOIMI_OK and "nothing at or
 * behind d_packed + packed_capacity is written" included.  A tile with factor 1, no flip and och == sch is the rectangle itself; a tile
 * that is a whole image gives qoimi_encode_images' stream.
 *   d_pixels, pixel_offsets, descs   as for qoimi_encode_images: ANY byte offsets, odd ones for 4-channel images too.  d_pixels is only read;
 *                  of an image nothing is read but the aligned 4-byte words that hold one of its bytes; an image that no tile names is not
 *                  read and its descs[i] is not even checked
 *   tiles          HOST qoimi_tile[n_tiles], in any order of image; they may overlap or coincide
 *   tile_descs_out HOST qoi_desc[n_tiles], may be NULL: the tiles' descriptors - with packed_off_out and stream_len_out all that
 *                  qoimi_decode_images and the gather calls need to serve the pack
 *   staging_bytes  device memory the call may hold for gathered pixels and strided streams: the staging arena of qoimi_encode_packed, counted in
 *                  qoimi_workspace_bytes [0] (56 + 8 bytes per tile for two tables beside it).  0: 1 GiB.  The plan (normative; qoi_amd/tiles.py:
 *                  plan): tile j's slot is tw * th * och rounded up to 256 plus qoimi_encode_bound of its descriptor rounded up to 256; sub-batches
 *                  are cut by qoi_amd/packplan.py: plan over those slots in tile order (a request smaller than one slot is raised to that slot).
 * Every sub-batch is one launch of the gather kernel over its tiles on `stream`, which writes them tightly packed into the pixel parts of their
 * slots, one qoimi_encode_images call as it is from there into the stream parts, qoimi_encode_status, and the pack's append - the loop of
 * qoimi_encode_images_packed.  SYNCHRONOUS, and as there: each sub-batch counts as ONE encode call for the LDS-order self-test; afterwards
 * qoimi_encode_status returns QOIMI_OK and never encodes again.
 * QOIMI_E_ARG, reported before anything is launched (the caller's buffers are untouched, qoimi_last_error names the cause): NULL ctx, d_pixels,
 * pixel_offsets, descs, tiles, d_packed_off or d_stream_len; n_images <= 0 or n_tiles <= 0; d_packed == NULL with a non-zero capacity; align not
 * a power of two in 1..256; channels not 0 / 3 / 4; a mode that is none of the four; tiles[j].image >= n_images; a rejected referenced
 * descriptor; a zero width or height; a rectangle that leaves its image; a factor outside 1..64; a flag bit other than the two flips;
 * reserved != 0; a factor above 16 with QOIMI_TILE_MODE; a referenced image whose last byte's address does not fit in a pointer; a referenced image whose bytes overlap [d_packed,
 * + packed_capacity); a sub-batch of the plan with 2^31 - 1 or more tiles of 256 work items of the gather kernel (an item is one aligned
 * 16-byte word of a tile's pixels at factor 1, else 1 to 16 per output pixel).  One call at a time per context, as everywhere.
 * Label maps (segmentation masks, instance ids, palette indices) - the mean of class 3 and class 7 is class 5 - take one of two further
 * values of `mode`, which this call alone accepts (qoimi_decode_thumbnails keeps rejecting them, and 2, 3 and every other value stay no
 * mode).  The definition (normative; qoi_amd/tiles.py: tile states it in Python).  S, R, width = cw, height = ch, f = factor, tw = ceil(cw /
 * f) and th = ceil(ch / f) are as above; R is taken at 4 bytes per pixel: a 3-channel source has alpha 255, and that alpha takes part.  The
 * block of output pixel (X, Y) is the box filter's, partial blocks at the right and bottom edge included: columns [X*f, min((X+1)*f, cw)),
 * nx of them, rows [Y*f, min((Y+1)*f, ch)), ny of them.  The block's centre pixel is column X*f + nx/2, row Y*f + ny/2 (the divisions floor).
 *   QOIMI_TILE_NEAREST  the output pixel is the centre pixel, byte for byte: a selection, at any factor 1..64
 *   QOIMI_TILE_MODE     the vote of QOIMI_FILTER_MODE (qoi_amd/mode.py: vote) over the block: whole pixels vote, all four bytes; the largest
 *                       count wins; of several winners the centre pixel wins if it is one of them, otherwise the lowest r << 24 | g << 16 |
 *                       b << 8 | a.  A tile with factor > 16 is QOIMI_E_ARG (a block holds at most 16 x 16 pixels, the limit of
 *                       QOIMI_FILTER_MODE), reported per tile behind the reserved != 0 check, before anything is launched
 * What follows the reduction is what follows the box filter: the flips, the conversion to och - 4 to 3 drops alpha AFTER the vote, so two
 * colours that differ in alpha alone vote apart; 3 to 4 sets 255 -, the reference encoder's stream byte for byte, the pack, the tables,
 * the capacity rules and the plan (the modes change no size: qoimi_tile_size has no mode argument).  factor == 1 is the rectangle itself
 * in both modes; a constant block gives the constant.  With f dividing cw and ch, a 4-channel source and och 4, a QOIMI_TILE_MODE tile is
 * what qoimi_decode_tensors gives with QOIMI_FILTER_MODE (u8, HWC) for the same rectangle at tw x th, byte for byte - its cells are then
 * the f-blocks and its nearest sample is Z*f + f/2 -, and a QOIMI_TILE_NEAREST tile is what QOIMI_FILTER_NEAREST gives.  Of the seven
 * levels of qoimi_tile_pyramid five (f = 1 .. 16) can vote; levels 5 and 6 (f = 32, 64) need QOIMI_TILE_NEAREST.  The two modes run a
 * gather kernel of their own over the same table; qoimi_tile_stats counts its launches in [1].
 * Not here: sources that are a pack (decode once with qoimi_decode_images), filters other than the box average, the selection and the vote,
 * a vote over blocks above 16 x 16, a vote per channel, a mode per tile, QOIMI_TILE_NEAREST / QOIMI_TILE_MODE in qoimi_decode_thumbnails
 * (qoimi_decode_tensors serves them), row-pitched sources, a channel count per tile. */
enum { QOIMI_TILE_NEAREST = 4, QOIMI_TILE_MODE = 5 };   /* 2 and 3 are not modes */
/* Tensors as the source (qoimi_tile.flags beside the two flips; accepted by qoimi_encode_tiles and qoimi_tile_size).  The two formats an
 * image really has on a device are a uint8 C x H x W tensor and a model's float output; with these bits the gather kernel converts them on
 * its way into the encoder's staging, and the caller runs no conversion passes and owns no interleaved u8 copy.
 *   QOIMI_TILE_SRC            the image this tile names is a TENSOR in the format the bits below give (none: u8, HWC - what it is without)
 *   QOIMI_TILE_SRC_CHW        planar: element (c, Y, X) at element index (c * h + Y) * w + X; without it HWC: (Y * w + X) * sch + c
 *   QOIMI_TILE_SRC_F16 / _BF16 / _F32   the dtype field, bits 6-7: QOIMI_TENSOR_U8 / _F16 / _BF16 / _F32 << 6 (element sizes 1 / 2 / 2 / 4)
 *   QOIMI_TILE_SRC_SYMMETRIC / _BYTES   the range field, bits 8-9, floats only.  0: UNIT, the element is in [0, 1]; SYMMETRIC: in [-1, 1];
 *                             BYTES: the element already is 0..255; 768 is not a range
 * descs[image] gives w, h and sch = 3 or 4 ELEMENTS per pixel (planes for CHW); pixel_offsets[image] stays a BYTE offset; the image takes
 * w * h * sch * element size bytes.  The conversion (normative; qoi_amd/tiles.py: convert states it in Python; qoi_amd/csrc/qoi_ingest_core.h
 * is the kernel's).  x is the element widened exactly to binary32 (binary16 and bfloat16 widen without rounding).
 *   UNIT       t = x * 255.0f, rounded to binary32
 *   SYMMETRIC  m = x * 127.5f, rounded; t = m + 127.5f, rounded: TWO roundings, never a fused multiply-add - the convention of qoimi_decode_tensors
 *   BYTES      t = x
 *   U8         the byte is the element
 * The byte is 0 if t is NaN or t <= 0 (which covers -inf and -0.0), 255 if t >= 255 (which covers +inf), otherwise t rounded to the nearest
 * integer, ties to even.  Every channel, alpha included, goes through the same conversion.  Whether subnormals are flushed cannot change a
 * byte: |t| < 0.5 gives 0 either way.  Let B be the h x w x sch byte image this defines: the tile is what qoimi_encode_tiles gives for B
 * without the bits - the rectangle, the flips, the conversion to och (4 to 3 drops alpha, 3 to 4 sets 255), the reference encoder's stream
 * byte for byte, the pack, the tables, the capacity rules, the staging plan and the slots.  No size changes.  At factor 1 all four values
 * of `mode` give the same bytes, as they do without the bits.  Of an image nothing is read but whole, naturally aligned elements (u8: the
 * aligned 4-byte words that hold one of its bytes); nothing of the caller's is written.
 * Limits, each QOIMI_E_ARG before anything is launched with the caller's buffers untouched, looked at per tile behind the checks above, in
 * this order: a SRC_* bit without QOIMI_TILE_SRC; range 768; a non-zero range with dtype U8; factor != 1 on a SRC tile; then, over the
 * call: some but not all tiles carry QOIMI_TILE_SRC (a call is a byte call or a tensor call; QOIMI_TILE_SRC alone marks a u8 HWC image
 * inside a tensor call, so formats still mix per image); two tiles that name the same image with different source bits; d_pixels +
 * pixel_offsets[image] not a multiple of the element size; the address-space and pack-overlap checks above, taken over the image's extent
 * in BYTES; a sub-batch of the plan with 2^31 - 1 or more tiles of 256 work items of the kernel (an item is four consecutive pixels of a
 * tile's output).  A tensor call runs a gather kernel of its own over the same table; qoimi_tile_stats counts its launches in [1].
 * Properties (qoi_amd/tiles.py asserts them).  A call whose tiles all carry QOIMI_TILE_SRC alone gives the pack of the same call without
 * the bit, byte for byte.  Round trip: for every byte v and each of F32, F16 and BF16, the element qoimi_decode_tensors writes for v
 * converts back to v with scale 1/255, bias 0 and UNIT; scale 2/255, bias -1 and SYMMETRIC; scale 1, bias 0 and BYTES.
 * Not here (of tensor sources): box, selection and vote over them (factor 1 only: convert once at factor 1, or decode the pack), a scale
 * and bias of the caller's, row-pitched tensors; integer dtypes other than u8 and one-plane (HW) sources are label sources: the
 * QOIMI_TILE_LABELS bits below. */
enum { QOIMI_TILE_SRC = 16, QOIMI_TILE_SRC_CHW = 32, QOIMI_TILE_SRC_F16 = 64, QOIMI_TILE_SRC_BF16 = 128, QOIMI_TILE_SRC_F32 = 192,
       QOIMI_TILE_SRC_SYMMETRIC = 256, QOIMI_TILE_SRC_BYTES = 512 };   /* bits 2, 3 and 10 stay unknown flag bits; 11-13: QOIMI_TILE_LABELS */
/* Label tensors as the source (qoimi_tile.flags beside the two flips; accepted by qoimi_encode_tiles and qoimi_tile_size): the ingest side
 * of QOIMI_TENSOR_I32 / _I64 in QOIMI_TENSOR_HW.  The label maps a device really holds are the int64 H x W argmax of a segmentation model,
 * an int32 instance map and a uint8 mask plane; with these bits they become a label pack - and a label pyramid - in one call, and the
 * caller clamps, narrows and interleaves nothing.
 *   QOIMI_TILE_LABELS                 the image this tile names is ONE PLANE of w x h elements: element (Y, X) at element index Y * w + X
 *   QOIMI_TILE_LABELS_I32 / _I64      the dtype field, bits 12-13: 0 u8, 1 little-endian two's-complement int32, 2 int64 (element size
 *                                     E = 1 / 4 / 8); 12288 is not a dtype
 * The plane is tightly packed at d_pixels + pixel_offsets[image], a BYTE offset that makes a multiple of E, and takes w * h * E bytes.
 * descs[image] gives w, h and colorspace; its channels (3 or 4, by the descriptor rules) only says what och is when the call's `channels`
 * is 0.  The conversion (normative; qoi_amd/tiles.py: labels_to_bytes states it in Python; qoi_amd/csrc/qoi_label_core.h is the kernel's).
 * The byte b of the element v is 0 for v < 0, 255 for v > 255, else v: saturation of the full 32- / 64-bit value - the high dword of an
 * int64 takes part: 2^32 is 255, not 0.  Saturation is SILENT: nothing counts or reports it, and an ignore index of -100 becomes class 0;
 * a caller who must know counts before the call.  Pixel (Y, X) of the byte image B (h x w x 4) is (b, b, b, 255).  The tile is what
 * qoimi_encode_tiles gives for B as a 4-channel byte image without the bits, in the call's `mode`: the rectangle, the reduction, the
 * flips, the conversion to och (4 to 3 drops the 255), the reference encoder's stream byte for byte, the pack, both tables,
 * tile_descs_out, the capacity rules, the staging plan and the slots.  No size changes: qoimi_tile_size needs no new argument.
 * Factor.  Unlike a QOIMI_TILE_SRC tile a label tile may reduce - with the label modes: QOIMI_TILE_NEAREST at factor 1..64,
 * QOIMI_TILE_MODE at factor 1..16 (the check above).  A label source is never averaged: QOIMI_THUMB_PLAIN / _ALPHA_WEIGHTED with
 * factor != 1 on a label tile is QOIMI_E_ARG.  At factor 1 all four modes give the same bytes, as everywhere.  All pixels of B are grey with
 * alpha 255, so the whole-pixel vote is the vote on b: among several winners the centre pixel wins if it is one, else the lowest b - the
 * rule of qoi_amd/mode.py: vote, unchanged.  Of a plane nothing is read but whole, naturally aligned elements (u8: the aligned 4-byte
 * words that hold one of its bytes); nothing of the caller's is written.
 * Properties (tests/test_label_ingest_model.py asserts them on qoi_amd/tiles.py).  (a) For a tensor with all values in 0..255, any dtype,
 * whole-image tiles at factor 1: qoimi_decode_tensors of the pack with QOIMI_FILTER_NEAREST, QOIMI_TENSOR_I64 and QOIMI_TENSOR_HW at the
 * image's size returns the tensor widened to int64.  (b) A u8 label call equals the byte call over B.  (c) With f dividing w and h, a
 * QOIMI_TILE_MODE label tile is what qoimi_decode_tensors gives with QOIMI_FILTER_MODE for the factor-1 pack at w/f x h/f - the statement
 * the byte tiles make above.
 * Limits, each QOIMI_E_ARG before anything is launched with the caller's buffers untouched, looked at per tile behind every check above
 * (those of QOIMI_TILE_SRC included), in this order: a LABELS_* dtype bit without QOIMI_TILE_LABELS; dtype 12288; QOIMI_TILE_LABELS
 * together with any QOIMI_TILE_SRC* bit; one of the two averaging modes with factor != 1 (qoimi_tile_size has no mode and does not look at
 * this one); then, over the call: some but not all tiles carry QOIMI_TILE_LABELS (a call is a byte call, a tensor call or a label call);
 * two tiles that name the same image with different label bits; d_pixels + pixel_offsets[image] not a multiple of E; the address-space
 * and pack-overlap checks above, taken over w * h * E bytes; a sub-batch of the plan with 2^31 - 1 or more tiles of 256 work items of the
 * kernel (an item is four consecutive pixels of a tile's output at factor 1, else 1 to 64 per output pixel as in the label modes).  A
 * label call runs a gather kernel of its own over the same table; qoimi_tile_stats counts its launches in [1].
 * 24-bit ids.  An instance map, a panoptic map (class * 1000 + instance) or a superpixel map has ids far above 255, which the byte rule
 * would all make 255.
 *   QOIMI_TILE_LABELS_ID24            bit 15, only together with QOIMI_TILE_LABELS: the elements of the plane are ids, not class indices
 * The plane, its dtype field, its alignment and its extent are those of a label tile.  The conversion (normative; qoi_amd/tiles.py:
 * label_ids_to_bytes states it in Python).  The id of the element v is 0 for v < 0, 2^24 - 1 for v > 2^24 - 1, else v: saturation of the
 * full 32- / 64-bit value - the high dword of an int64 takes part: 2^32 + 5 is 2^24 - 1, not 5 - and silent, as the byte rule is.  Pixel
 * (Y, X) of B is (id & 255, (id >> 8) & 255, id >> 16, 255) - as a dword id | 0xFF000000 -: the COCO panoptic convention
 * id = R + 256 * G + 256^2 * B, so a panoptic PNG converted to QOI already is such a pack.  A u8 plane with the bit gives (v, 0, 0, 255):
 * it is allowed so that a mask can join an id pack.  Everything behind B is what a label tile does without the bit: the rectangle, the
 * flips, och (4 to 3 drops the 255), factor 1, QOIMI_TILE_NEAREST at factor 1..64 and QOIMI_TILE_MODE at 1..16, never the averaging
 * modes, the reference encoder's stream byte for byte, the pack, the tables, the plan and the slots.  The pixels are no longer grey, so
 * the vote is the whole-pixel vote as it stands: among several winners without the centre pixel the lowest
 * r << 24 | g << 16 | b << 8 | a wins - the order of the id's bytes from the LOW byte up, not the lowest id: of the ids 256 and 1 it is
 * 256, which is (0, 1, 0, 255).  The rule of qoi_amd/mode.py: vote is not changed.
 * Properties (tests/test_label_id_model.py asserts them on qoi_amd/tiles.py and qoi_amd/tensors.py).  (a) For a plane with all values in
 * 0..2^24 - 1, any dtype, whole-image tiles at factor 1: qoimi_decode_tensors of the pack with QOIMI_FILTER_NEAREST, QOIMI_TENSOR_I64 and
 * QOIMI_TENSOR_HW_ID24 at the image's size returns the plane widened to int64.  (b) A call without the bit gives the bytes it gave.  (c)
 * With f dividing w and h, an ID24 QOIMI_TILE_MODE tile decodes to what QOIMI_FILTER_MODE gives from the factor-1 pack at w/f x h/f.
 * Its checks, where the label checks stand: bit 15 without QOIMI_TILE_LABELS is "a LABELS_* bit without QOIMI_TILE_LABELS"; "two tiles
 * that name the same image with different label bits" compares bit 15 too - an image is bytes or ids -; images with and without the bit
 * mix in one label call.  The gather kernel is the label call's, with the id variant as three more values of an entry's dtype field.
 * Not here (of label sources): a count of saturated elements, a remap table, i16 / u16, ids above 2^24 - 1 (alpha is 255), float class
 * maps, a plane of a CHW tensor chosen by index (offset it yourself), row-pitched planes, label and tensor tiles in one call. */
enum { QOIMI_TILE_LABELS = 2048, QOIMI_TILE_LABELS_I32 = 4096, QOIMI_TILE_LABELS_I64 = 8192 };
enum { QOIMI_TILE_LABELS_ID24 = 32768 };   /* bit 15: 24-bit ids over r, g and b; bit 14 stays an unknown flag bit */
/* dtype field, bits 12-13: 0 u8, 1 i32, 2 i64; 12288 is not a dtype.  Bit 10, bit 14 and bits 16 up stay unknown flag bits; bit 15: QOIMI_TILE_LABELS_ID24. */
typedef struct {                 /* 32 bytes, offsets 0/4/8/12/16/20/24/28 */
    unsigned int image;          /* index into the call's images */
    unsigned int x, y;           /* top-left corner of the source rectangle */
    unsigned int width, height;  /* both >= 1; the rectangle lies inside the image */
    unsigned int factor;         /* 1..64 */
    unsigned int flags;          /* QOIMI_CROP_FLIP_X / _Y; no other bit */
    unsigned int reserved;       /* 0 */
} qoimi_tile;
int qoimi_encode_tiles(qoimi_ctx *ctx, const void *d_pixels, const size_t *pixel_offsets /* host */, const qoi_desc *descs /* host */, int n_images,
                       int channels /* 0, 3, 4 */, const qoimi_tile *tiles /* host */, int n_tiles, int mode /* QOIMI_THUMB_PLAIN / _ALPHA_WEIGHTED, QOIMI_TILE_NEAREST / _MODE */,
                       unsigned align, void *d_packed, size_t packed_capacity,
                       unsigned long long *d_packed_off /* device, n_tiles + 1 */, int *d_stream_len /* device, n_tiles */, size_t staging_bytes,
                       unsigned long long *packed_off_out /* host, may be NULL */, int *stream_len_out /* host, may be NULL */,
                       qoi_desc *tile_descs_out /* host, n_tiles, may be NULL */, void *stream);

/* tw = ceil(tile->width / factor), th = ceil(tile->height / factor); returns tw * th * och (och = channels, or desc->channels when channels is
 * 0) - the bytes of the tile's pixels - or 0 if desc is rejected, tile is NULL, has a zero width or height, leaves the image of desc, has a
 * factor outside 1..64, an unknown flag bit or reserved != 0, or channels is not 0 / 3 / 4 (tw / th are then left alone; tile->image is not
 * looked at).  Pure host arithmetic: no context, no GPU.  tw / th may be NULL. */
size_t qoimi_tile_size(const qoi_desc *desc, const qoimi_tile *tile, int channels, unsigned *tw, unsigned *th);

/* The tiles of a pyramid of `levels` levels over one image, in the order level, row, column.  Level l = 0 .. levels - 1 has f = 2^l; its
 * image is Lw = ceil(w / f) by Lh = ceil(h / f) and is cut into ceil(Lh / tile_h) rows of ceil(Lw / tile_w) tiles; tile (l, row, col) is
 * x = col * tile_w * f, y = row * tile_h * f, width = min(tile_w * f, w - x), height = min(tile_h * f, h - y), factor = f, image, flags and
 * reserved 0.  Every x and y is a multiple of f, so the tiles of level l are exactly the qoimi_decode_thumbnails reduction of the whole image
 * at 2^l cut on the grid: each level is ONE rounding from the full-resolution pixels, not a chain of halvings.  Returns the number of tiles
 * and fills out[0 .. that) when out is not NULL; QOIMI_E_ARG for a rejected descriptor, tile_w or tile_h of 0 or above 2^24, levels outside
 * 1..7, a non-NULL out with cap too small, more than 2^31 - 1 tiles.  Pure host arithmetic: no context, no GPU. */
int qoimi_tile_pyramid(const qoi_desc *desc, unsigned tile_w, unsigned tile_h, unsigned levels, qoimi_tile *out /* may be NULL */, int cap);

/* Of the context's last qoimi_encode_tiles call: [0] sub-batches, [1] launches of the gather kernel (it has no entry in qoimi_kernel_name),
 * [2] bytes of the staging the call planned for (its largest sub-batch), [3] images referenced. */
void qoimi_tile_stats(qoimi_ctx *ctx, long long out[4]);

/* What makes a pack self-describing: the header of every stream, read on the device and parsed by the rules of qoi.h:497-521.
 *   stream_offsets, sizes  HOST arrays as for qoimi_decode_images
 *   descs_out      HOST qoi_desc[n_streams]: filled for every stream of 22 bytes or more, valid or not (as qoi_decode fills *desc before
 *                  it validates; a shorter stream leaves its entry untouched, as qoi_decode returns before it touches *desc)
 *   first_bad      HOST, may be NULL: the lowest index that fails, -1 if none
 * QOIMI_OK if every stream passes (size >= 22, magic, non-zero width / height, channels 3 / 4, colorspace <= 1, the pixel cap), else
 * QOIMI_E_ARG.  Synchronous.  With it (d_packed, offsets, sizes) is all a caller has to keep: read_descs -> allocate -> decode_images. */
int qoimi_read_descs(qoimi_ctx *ctx, const void *d_streams, const size_t *stream_offsets, const int *sizes, int n_streams,
                     qoi_desc *descs_out /* host */, int *first_bad /* host, may be NULL */, void *stream);

/* What is in the streams of a pack, and whether they are intact: the chunk walk of every stream WITHOUT decoding it - no pixel state, no
 * colour table, no output image; a function of the stream bytes alone.  qoi_decode and the decode calls above keep the reference's
 * leniency (a cut stream decodes into repeated pixels, a chunk may reach into the trailer, surplus chunks and a wrong end marker are
 * ignored, all with QOIMI_OK); this call is the strict counterpart.
 * The walk (normative; qoi_amd/streaminfo.py: inspect_stream states it in Python): p = 14, end = size - 8; while p < end read b = s[p]:
 *   0xFE -> RGB, 4 bytes;  0xFF -> RGBA, 5 bytes;  b >> 6 == 0 -> INDEX, 1 byte;  == 1 -> DIFF, 1 byte;  == 2 -> LUMA, 2 bytes;
 *   == 3 -> RUN, 1 byte, (b & 63) + 1 pixels; every other chunk is 1 pixel.  Count the chunk, add its pixels, advance p by its length.
 * walk_end = p.  These are the tag rules of qoi.h:547-575, but the walk is bounded by the BYTES, not by width*height as the reference's
 * loop is: only so can it tell a stream that is short of pixels from one that has too many.  A chunk that starts below size - 8 ends
 * below size - 3, so nothing outside [offset, offset + size) is read - but for the aligned 4-byte words that hold a first or last byte. */
enum { QOIMI_OP_INDEX = 0, QOIMI_OP_DIFF, QOIMI_OP_LUMA, QOIMI_OP_RUN, QOIMI_OP_RGB, QOIMI_OP_RGBA };
enum {
    QOIMI_SI_TOO_SHORT      = 1,   /* size < 22: nothing was read, every other field is 0 */
    QOIMI_SI_HEADER_BAD     = 2,   /* fails the rules qoimi_read_descs applies (qoi.h:497-521) */
    QOIMI_SI_PIXELS_SHORT   = 4,   /* pixels < width*height: the decoder repeats the last pixel (qoi.h:544) */
    QOIMI_SI_PIXELS_OVER    = 8,   /* pixels > width*height: the decoder clips a run / ignores chunks */
    QOIMI_SI_LAST_CHUNK_CUT = 16,  /* walk_end > size - 8: the last chunk reaches into the final 8 bytes */
    QOIMI_SI_NO_END_MARKER  = 32,  /* the final 8 bytes are not 0,0,0,0,0,0,0,1 (qoi.h:103,339) */
    QOIMI_SI_REPEATED_INDEX = 64   /* repeat_index != 0 (qoi.h:118-119) */
};
typedef struct {                    /* 64 bytes, offsets 0/8/16/40/44/48/52 */
    unsigned long long pixels;      /* pixels the chunks produce, runs counted in full, NOT clipped to width*height */
    unsigned long long run_pixels;  /* of those, produced by QOI_OP_RUN chunks */
    unsigned int ops[6];            /* chunks by kind, indexed by QOIMI_OP_* */
    unsigned int repeat_index;      /* INDEX chunks that directly follow an INDEX chunk with the same byte */
    unsigned int walk_end;          /* byte offset in the stream where the walk ends (size-8 ... size-4) */
    unsigned int flags;             /* QOIMI_SI_* */
    unsigned int reserved[3];       /* 0 */
} qoimi_stream_info;

/*   stream_offsets, sizes  HOST arrays as for qoimi_decode_images: any byte offsets, any order; ranges may overlap or coincide
 *   infos_out      HOST qoimi_stream_info[n_streams]
 *   first_flagged  HOST, may be NULL: the lowest index with flags != 0, -1 if none
 * PIXELS_SHORT / PIXELS_OVER are evaluated only when the header passes (against the 64-bit product width*height); a stream of 22 bytes or
 * more with a bad header is walked all the same.  A stream is conforming when flags == 0.
 * Synchronous.  QOIMI_OK when the inspection ran, whatever it found (n_streams == 0 included); QOIMI_E_ARG for a NULL ctx, stream_offsets,
 * sizes or infos_out, d_streams == NULL with n_streams > 0, n_streams < 0 or a negative size: nothing is launched, infos_out is untouched.
 * Cost: the stream bytes are read twice by kernels that do nothing else; workspace (counted in qoimi_workspace_bytes [1]) is 1/32 of the
 * stream bytes plus 69 bytes per 16 KiB block of a stream and 16 per stream.  One call at a time per context, as everywhere. */
int qoimi_inspect_streams(qoimi_ctx *ctx, const void *d_streams, const size_t *stream_offsets, const int *sizes, int n_streams,
                          qoimi_stream_info *infos_out /* host */, int *first_flagged /* host, may be NULL */, void *stream);

/* Are two sets of device images equal, pixel by pixel?  (The comparison is stated in Python by qoi_amd/imagediff.py: diff.)
 *   a_offsets, b_offsets  HOST size_t[n_images]: image i of side A lies tightly packed at d_a + a_offsets[i] - descs[i].width * height pixels
 *                  of ca bytes, ca = a_channels, or descs[i].channels when a_channels is 0 (the convention of qoimi_decode_images' `channels`);
 *                  side B the same with b_channels.  ANY byte offsets, in any order; A and B may be the same buffer and ranges may overlap
 *                  (nothing is written).  Not one byte outside an image's range influences the result; reads may touch the aligned 4-byte
 *                  words that hold a first or last byte.
 *   descs          HOST qoi_desc[n_images]: every one must pass the rules of qoi.h:364-372 (colorspace takes no part in the comparison)
 *   diffs_out      HOST qoimi_image_diff[n_images]
 *   first_diff     HOST, may be NULL: the lowest index with flags != 0, -1 if none
 * Two pixels are equal when their first min(ca, cb) bytes are: an RGB buffer against an RGBA buffer compares r, g, b.
 * Synchronous.  QOIMI_OK whenever the comparison ran, whatever it found; QOIMI_E_ARG for a NULL ctx, d_a, d_b, a_offsets, b_offsets, descs or
 * diffs_out, n_images <= 0, a_channels or b_channels not 0, 3 or 4, a rejected descriptor: nothing is launched, diffs_out is untouched.
 * Cost: every byte of both sides is read once by one launch for all images (cmp_pixels), a second launch of a thread per image reads the
 * pixels at the first differences (cmp_first); 64 bytes of workspace per image (counted in qoimi_workspace_bytes [1]). */
enum { QOIMI_DIFF_PIXELS = 1,          /* mismatched != 0 */
       QOIMI_DIFF_HEADER = 2 };        /* qoimi_verify_images only: see there; the image was not decoded, every other field is 0 / ~0 */
typedef struct {                        /* 32 bytes, offsets 0/8/16/20/24/28 */
    unsigned long long mismatched;      /* pixels that differ */
    unsigned long long first;           /* row-major index of the first differing pixel, ~0ull if none */
    unsigned int want;                  /* pixel `first` of side A, bytes r,g,b,a little-endian; a channel the buffer does not hold reads 0xFF; 0 if none */
    unsigned int got;                   /* the same of side B */
    unsigned int flags;                 /* QOIMI_DIFF_* */
    unsigned int reserved;              /* 0 */
} qoimi_image_diff;
int qoimi_compare_images(qoimi_ctx *ctx,
                         const void *d_a, const size_t *a_offsets /* host */, int a_channels,
                         const void *d_b, const size_t *b_offsets /* host */, int b_channels,
                         const qoi_desc *descs /* host */, int n_images,
                         qoimi_image_diff *diffs_out /* host */, int *first_diff /* host, may be NULL */, void *stream);

/* Do these streams decode back to exactly these pixels?  diffs_out[i] is DEFINED as: decode stream i (sizes[i] bytes at d_streams +
 * stream_offsets[i]) as qoi_decode does, with its leniency (qoi.h:488-590), to descs[i].channels output channels; take that decode as side B
 * and the caller's image i (tightly packed at d_pixels + pixel_offsets[i], descs[i].channels bytes per pixel) as side A of
 * qoimi_compare_images with ca = cb = descs[i].channels.  The caller never owns the decode: the context decodes consecutive sub-batches of
 * whole images into a staging arena of its own and compares each in place; one table of results travels to the host at the end.
 *   QOIMI_DIFF_HEADER  a stream shorter than 22 bytes, one whose header fails the rules of qoimi_read_descs, or whose header differs from
 *                  descs[i] in width, height, channels or colorspace is not decoded: this flag alone, first = ~0, every other field 0.  Its
 *                  neighbours are unaffected.
 *   staging_bytes  device memory the call may hold for decoded pixels (an arena of the context, counted in qoimi_workspace_bytes [1]; it grows
 *                  when a call needs more and is allocated as the largest sub-batch of the call's plan plus a page, no slack).  0: 1 GiB.
 *                  The staging is decoded at ONE channel count per call, och = 3 if every descs[i].channels is 3, else 4 (alpha is compared
 *                  exactly where the source image has it, and got reports a 3-channel image's alpha as 0xFF).  The sub-batch plan
 *                  (normative; qoi_amd/packplan.py: plan over width * height * och): a slot is width * height * och rounded up to 256
 *                  bytes, images are taken in order, a sub-batch closes when the next slot would not fit in staging_bytes; a request
 *                  smaller than one slot is raised to that slot.  An image flagged QOIMI_DIFF_HEADER keeps its place and its slot in the
 *                  plan - the plan is a function of descs and staging_bytes alone - and is left out of its sub-batch's decode and compare.
 * Every sub-batch is one qoimi_decode_images call as it is (same bit-exactness for EVERY input stream), then the compare kernels on `stream`.
 * Synchronous.  QOIMI_OK when the verification ran, whatever it found; the code of a decode sub-call that failed ends the call.  QOIMI_E_ARG
 * for a NULL ctx, d_pixels, pixel_offsets, descs, d_streams, stream_offsets, sizes or diffs_out, n_images <= 0, a negative size, a rejected
 * descs[i]: reported before anything is launched, diffs_out is untouched.  d_pixels and d_streams are only read.
 * The sub-batches count as decode calls for everything a context's decode calls choose by what came before (the single-pass path of calls of
 * a few images, segment sizes, qoimi_decode_stats - which holds the last sub-batch's), as the sub-batches of qoimi_encode_packed count as
 * encode calls.  One call at a time per context, as everywhere. */
int qoimi_verify_images(qoimi_ctx *ctx,
                        const void *d_pixels, const size_t *pixel_offsets /* host */, const qoi_desc *descs /* host */, int n_images,
                        const void *d_streams, const size_t *stream_offsets /* host */, const int *sizes /* host */,
                        size_t staging_bytes,
                        qoimi_image_diff *diffs_out /* host */, int *first_diff /* host, may be NULL */, void *stream);

/* Every image of a pack at 1/f of its size, without the caller ever owning the full-size images.  QOI cannot be decoded at reduced size (every
 * pixel depends on the one before), so the streams are decoded in full - into a staging arena of the context, sub-batch by sub-batch - and each
 * sub-batch is reduced on the device by an exact integer box filter.
 * The result (normative; qoi_amd/thumbs.py: thumbnail states it in Python): decode stream i exactly as qoimi_decode_images does (same leniency,
 * bit-exact for EVERY input stream) to och = channels, or descs[i].channels when channels is 0 (the same for all images of the call), which gives
 * D of w x h pixels.  With f = factors[i], tw = ceil(w / f), th = ceil(h / f), output pixel (X, Y) covers the source block x in [X*f, min(w,
 * X*f+f)), y in [Y*f, min(h, Y*f+f)) of cnt pixels; S_c is the sum of channel c over the block.  Divisions are integer divisions (floor).
 *   QOIMI_THUMB_PLAIN           every output channel is (S_c + cnt/2) / cnt - a half rounds up
 *   QOIMI_THUMB_ALPHA_WEIGHTED  where och == 4: A = S_a, output alpha is (A + cnt/2) / cnt; if A > 0, r, g and b are (sum(c_k * a_k) + A/2) / A
 *                               over the block's pixels k, if A == 0 they are the PLAIN value.  With och == 3 this mode is PLAIN.
 * f == 1 reproduces the decode byte for byte in both modes.  Every sum fits in 32 bits (64 * 64 * 255 * 255 < 2^32).
 *   stream_offsets, sizes, descs, channels  HOST arrays / value as for qoimi_decode_images
 *   factors        HOST unsigned[n_images], each 1..64
 *   thumb_offsets  HOST size_t[n_images]: thumbnail i is written tightly packed, tw * th * och bytes (qoimi_thumbnail_size), at d_thumbs +
 *                  thumb_offsets[i].  ANY byte offsets in any order; not one byte beside a thumbnail is written; ranges must not overlap
 *   staging_bytes  device memory the call may hold for decoded pixels (the arena qoimi_verify_images uses, counted in qoimi_workspace_bytes [1],
 *                  allocated as the largest sub-batch of the call's plan plus a page, no slack).  0: 1 GiB.  The staging always holds 4 bytes per
 *                  pixel (a 3-channel stream decodes with alpha 255, which a 3-channel thumbnail does not store).  The sub-batch plan
 *                  (normative; qoi_amd/packplan.py: plan over width * height * 4): a slot is width * height * 4 rounded up to 256 bytes, images
 *                  are taken in order, a sub-batch closes when the next slot would not fit in staging_bytes; a request smaller than one slot is
 *                  raised to that slot, so every sub-batch holds at least one image.
 * Every sub-batch is one qoimi_decode_images call as it is, at 4 output channels, then one launch of the reduction kernel on `stream`.
 * SYNCHRONOUS: returns when every thumbnail is written.  The code of a decode sub-call that failed ends the call.  QOIMI_E_ARG for a NULL ctx,
 * d_streams, stream_offsets, sizes, descs, factors, d_thumbs or thumb_offsets, n_images <= 0, sizes[i] < 22, a rejected descriptor, channels not
 * 0 / 3 / 4, mixed output channel counts, a factor outside 1..64, a mode that is neither of the two, overlapping output ranges, a sub-batch
 * of the plan with 2^31 - 1 or more tiles of 256 work items of the reduction kernel (an output pixel is 1 to 16 items; no staging a device can hold
 * comes near it): reported before anything is launched, the caller's buffers are untouched.  The sub-batches count as decode calls of the context, as those of
 * qoimi_verify_images do.  One call at a time per context, as everywhere. */
enum { QOIMI_THUMB_PLAIN = 0, QOIMI_THUMB_ALPHA_WEIGHTED = 1 };
int qoimi_decode_thumbnails(qoimi_ctx *ctx, const void *d_streams, const size_t *stream_offsets /* host */, const int *sizes /* host */,
                            const qoi_desc *descs /* host */, int n_images, int channels /* 0, 3, 4 */,
                            const unsigned *factors /* host, n_images, each 1..64 */, int mode,
                            void *d_thumbs, const size_t *thumb_offsets /* host */, size_t staging_bytes, void *stream);

/* tw = ceil(width / factor), th = ceil(height / factor); returns tw * th * channels - the bytes of the thumbnail - or 0 if desc is rejected,
 * factor is not in 1..64 or channels is not 3 / 4 (tw / th are then left alone).  Pure host arithmetic: no context, no GPU.  tw / th may be NULL. */
size_t qoimi_thumbnail_size(const qoi_desc *desc, unsigned factor, int channels, unsigned *tw, unsigned *th);

/* Of the context's last qoimi_decode_thumbnails call: [0] sub-batches decoded, [1] launches of the reduction kernel (it has no entry in
 * qoimi_kernel_name), [2] bytes of the staging the call planned for (its largest sub-batch), [3] 0. */
void qoimi_thumbnail_stats(qoimi_ctx *ctx, long long out[4]);

/* Rectangles of a pack's images, as they are, without the caller ever owning the full-size images: a tile server cuts a large scan into tiles, a
 * training loader takes one or several crops per image, often mirrored.  QOI cannot be decoded from the middle (every pixel depends on the one
 * before), so a referenced stream is decoded from its start - into a staging arena of the context, sub-batch by sub-batch - but only down to the
 * last row any crop needs, and the rectangles are gathered from there on the device.
 * The result (normative; qoi_amd/crops.py: crop states it in Python): decode stream crops[j].image exactly as qoimi_decode_images does (same
 * leniency, bit-exact for EVERY input stream) to och = channels, or the images' own channel count when channels is 0 (then the same for all
 * REFERENCED images), which gives D of h rows of w pixels.  Output j is D[y .. y + height) x [x .. x + width), its rows in reverse order with
 * QOIMI_CROP_FLIP_Y and its columns with QOIMI_CROP_FLIP_X, written tightly packed row-major, width * height * och bytes (qoimi_crop_size), at
 * d_out + out_offsets[j].
 *   stream_offsets, sizes, descs, channels  HOST arrays / value as for qoimi_decode_images.  An image that no crop names is NOT decoded and its
 *                  sizes[i] and descs[i] are not even checked
 *   crops          HOST qoimi_crop[n_crops], in any order of image; several may name the same image, their rectangles may overlap or coincide
 *   out_offsets    HOST size_t[n_crops]: ANY byte offsets in any order; not one byte beside an output is written (two outputs may share an
 *                  aligned word: no word is ever read and written back); ranges must not overlap
 *   staging_bytes  device memory the call may hold for decoded pixels (the arena qoimi_verify_images and qoimi_decode_thumbnails use, counted in
 *                  qoimi_workspace_bytes [1], allocated as the largest sub-batch of the call's plan plus a page, no slack).  0: 1 GiB.  The
 *                  staging always holds 4 bytes per pixel.  The plan (normative; qoi_amd/crops.py: plan): the referenced images are taken in
 *                  ascending index order; rows_i is the maximum of y + height over the crops of image i; a slot is width_i * rows_i * 4
 *                  rounded up to 256 bytes; sub-batches are cut by qoi_amd/packplan.py: plan over those slots (a request smaller than one slot
 *                  is raised to that slot).  A 256-row band at the top of a 16384 x 16384 scan is staged in 16 MiB instead of 1 GiB.
 * Every sub-batch is one qoimi_decode_images call as it is, at 4 output channels and with each descriptor's height replaced by rows_i (the
 * decoder decodes to the descriptor it is given, so this is exactly the first rows_i rows of the full decode), then one launch of the gather
 * kernel over all crops of the sub-batch's images on `stream`.
 * SYNCHRONOUS: returns when every output is written.  The code of a decode sub-call that failed ends the call.  QOIMI_E_ARG for a NULL ctx,
 * d_streams, stream_offsets, sizes, descs, crops, d_out or out_offsets, n_images <= 0, n_crops <= 0, channels not 0 / 3 / 4, crops[j].image >=
 * n_images, a zero width or height, a rectangle that leaves its image, a flag bit other than the two, a referenced stream shorter than 22 bytes,
 * a rejected referenced descriptor, mixed channel counts among the referenced images when channels is 0, overlapping output ranges, an output
 * whose last byte's address d_out + out_offsets[j] + size - 1 does not fit in a pointer, a sub-batch
 * of the plan with 2^31 - 1 or more tiles of 256 work items of the gather kernel (an item is one aligned 16-byte word of an output): reported
 * before anything is launched, the caller's buffers are untouched.  The sub-batches count as decode calls of the context, as those of
 * qoimi_verify_images do.  One call at a time per context, as everywhere. */
enum { QOIMI_CROP_FLIP_X = 1, QOIMI_CROP_FLIP_Y = 2 };
typedef struct {                 /* 24 bytes, offsets 0/4/8/12/16/20 */
    unsigned int image;          /* index into the call's images */
    unsigned int x, y;           /* top-left corner in the source image */
    unsigned int width, height;  /* both >= 1; x + width <= image width, y + height <= image height */
    unsigned int flags;          /* QOIMI_CROP_FLIP_* ; no other bit */
} qoimi_crop;
int qoimi_decode_crops(qoimi_ctx *ctx, const void *d_streams, const size_t *stream_offsets /* host */, const int *sizes /* host */,
                       const qoi_desc *descs /* host */, int n_images, int channels /* 0, 3, 4 */,
                       const qoimi_crop *crops /* host */, int n_crops,
                       void *d_out, const size_t *out_offsets /* host, n_crops */, size_t staging_bytes, void *stream);

/* width * height * channels - the bytes of the crop's output - or 0 if desc is rejected, crop is NULL, has a zero width or height, leaves the
 * image of desc or carries an unknown flag bit, or channels is not 3 / 4 (crop->image is not looked at).  Pure host arithmetic: no context, no GPU. */
size_t qoimi_crop_size(const qoi_desc *desc, const qoimi_crop *crop, int channels);

/* Of the context's last qoimi_decode_crops call: [0] sub-batches decoded, [1] launches of the gather kernel (it has no entry in
 * qoimi_kernel_name), [2] bytes of the staging the call planned for (its largest sub-batch), [3] images decoded (the referenced ones). */
void qoimi_crop_stats(qoimi_ctx *ctx, long long out[4]);

/* Rectangles of a pack's images resampled to caller-chosen sizes, without the caller ever owning the full-size images or the unscaled rectangles: a
 * training loader wants every sample of a batch at one fixed size (random-resized-crop, often mirrored), a tile server a tile of fixed size at
 * any zoom.  The common generalisation of qoimi_decode_thumbnails and qoimi_decode_crops: with out_width x out_height equal to width x height it is
 * qoimi_decode_crops byte for byte, and where width and height are the same integer multiple f of out_width and out_height it is the
 * qoimi_decode_thumbnails reduction of the rectangle at f, byte for byte in both modes.
 * The result (normative; qoi_amd/resize.py: resize states it in Python): decode stream items[j].image exactly as qoimi_decode_images does (same
 * leniency, bit-exact for EVERY input stream) to och = channels, or the images' own channel count when channels is 0 (then the same for all
 * REFERENCED images), which gives D of h rows of w pixels.  R = D[y .. y + height) x [x .. x + width), cw = width, rh = height, ow = out_width,
 * oh = out_height; all arithmetic is integer, every division floors.  Output column X weighs source column k of R with wx(X, k) = max(0,
 * min((X+1)*cw, (k+1)*ow) - max(X*cw, k*ow)) - the overlap of [X*cw, (X+1)*cw) with [k*ow, (k+1)*ow), summing to cw over k; wy(Y, r) is the same
 * with rh, oh and sums to rh.  T = cw * rh, N_c = sum over r, k of wy(Y, r) * wx(X, k) * R[r][k].c.
 *   QOIMI_RESIZE_PLAIN           every channel of output pixel (X, Y) is (N_c + T/2) / T: ONE rounding, no rounded intermediate between a
 *                                horizontal and a vertical pass
 *   QOIMI_RESIZE_ALPHA_WEIGHTED  where och == 4: A = N_a, output alpha is (A + T/2) / T; if A > 0, r, g and b are (sum wy * wx * c * a + A/2) / A,
 *                                if A == 0 they are the PLAIN value.  With och == 3 this mode is PLAIN.
 * The oh x ow result has its rows in reverse order with QOIMI_RESIZE_FLIP_Y and its columns with QOIMI_RESIZE_FLIP_X (the weights are symmetric:
 * this is the resampled mirrored rectangle) and is written tightly packed row-major, ow * oh * och bytes (qoimi_resize_size), at d_out +
 * out_offsets[j].  T < 400 000 000, N_c <= 255 * T < 2^37, the alpha-weighted sums are below 2^45.  Upscaling is allowed in either axis; downscaling
 * stops at 64 per axis (width <= 64 * out_width, height <= 64 * out_height - the limit of qoimi_decode_thumbnails), so an output pixel overlaps
 * at most 65 x 65 source pixels.
 *   stream_offsets, sizes, descs, channels  HOST arrays / value as for qoimi_decode_images.  An image that no item names is NOT decoded and its
 *                  sizes[i] and descs[i] are not even checked
 *   items          HOST qoimi_resize[n_items], in any order of image; several may name the same image, their rectangles may overlap or coincide
 *   out_offsets    HOST size_t[n_items]: ANY byte offsets in any order; not one byte beside an output is written (two outputs may share an
 *                  aligned word: no word is ever read and written back); ranges must not overlap
 *   staging_bytes  as for qoimi_decode_crops: the arena qoimi_verify_images, qoimi_decode_thumbnails and qoimi_decode_crops use, counted in
 *                  qoimi_workspace_bytes [1], allocated as the largest sub-batch of the call's plan plus a page; 4 bytes per pixel; 0: 1 GiB.
 *                  The plan is that of qoimi_decode_crops over the items' rectangles (normative; qoi_amd/resize.py: plan): the referenced
 *                  images in ascending order, rows_i the maximum of y + height over the items of image i, slots of width_i * rows_i * 4 rounded
 *                  up to 256 bytes, sub-batches cut by qoi_amd/packplan.py: plan (a request smaller than one slot is raised to that slot).
 * Every sub-batch is one qoimi_decode_images call as it is, at 4 output channels and with each descriptor's height replaced by rows_i, then one
 * launch of the filter kernel over all items of the sub-batch's images on `stream`.
 * SYNCHRONOUS: returns when every output is written.  The code of a decode sub-call that failed ends the call.  QOIMI_E_ARG for a NULL ctx,
 * d_streams, stream_offsets, sizes, descs, items, d_out or out_offsets, n_images <= 0, n_items <= 0, channels not 0 / 3 / 4, a mode that is
 * neither of the two, items[j].image >= n_images, a zero width, height, out_width or out_height, a rectangle that leaves its image, width > 64 *
 * out_width or height > 64 * out_height, a flag bit other than the two, a referenced stream shorter than 22 bytes, a rejected referenced
 * descriptor, mixed channel counts among the referenced images when channels is 0, overlapping output ranges, an output whose last byte's
 * address does not fit in a pointer, a sub-batch of the plan with 2^31 - 1 or more tiles of 256 work items of the filter kernel (an output pixel
 * is 1 to 16 work items): reported before anything is launched, the caller's buffers are untouched.  The sub-batches count as decode calls of the
 * context, as those of qoimi_verify_images do.  One call at a time per context, as everywhere. */
enum { QOIMI_RESIZE_FLIP_X = 1, QOIMI_RESIZE_FLIP_Y = 2 };
enum { QOIMI_RESIZE_PLAIN = 0, QOIMI_RESIZE_ALPHA_WEIGHTED = 1 };
typedef struct {                 /* 32 bytes, offsets 0/4/8/12/16/20/24/28 */
    unsigned int image;          /* index into the call's images */
    unsigned int x, y;           /* top-left corner of the source rectangle */
    unsigned int width, height;  /* both >= 1; x + width <= image width, y + height <= image height */
    unsigned int out_width, out_height;  /* both >= 1; width <= 64 * out_width, height <= 64 * out_height */
    unsigned int flags;          /* QOIMI_RESIZE_FLIP_* ; no other bit */
} qoimi_resize;
int qoimi_decode_resized(qoimi_ctx *ctx, const void *d_streams, const size_t *stream_offsets /* host */, const int *sizes /* host */,
                         const qoi_desc *descs /* host */, int n_images, int channels /* 0, 3, 4 */,
                         const qoimi_resize *items /* host */, int n_items, int mode,
                         void *d_out, const size_t *out_offsets /* host, n_items */, size_t staging_bytes, void *stream);

/* out_width * out_height * channels - the bytes of the item's output - or 0 if desc is rejected, item is NULL, has a zero width or height in or
 * out, leaves the image of desc, reduces by more than 64 in an axis or carries an unknown flag bit, channels is not 3 / 4, or the product does
 * not fit a size_t (item->image is not looked at).  Pure host arithmetic: no context, no GPU. */
size_t qoimi_resize_size(const qoi_desc *desc, const qoimi_resize *item, int channels);

/* Of the context's last qoimi_decode_resized call: [0] sub-batches decoded, [1] launches of the filter kernel (it has no entry in
 * qoimi_kernel_name), [2] bytes of the staging the call planned for (its largest sub-batch), [3] images decoded (the referenced ones). */
void qoimi_resize_stats(qoimi_ctx *ctx, long long out[4]);

/* qoimi_decode_resized with an antialiased bilinear (triangle) filter in place of the area filter: what torchvision Resize, PIL BILINEAR and DALI
 * resample with by default.  The area filter is the right one for reducing; enlarging with it is nearest-neighbour with soft edges, so a
 * random-resized-crop that takes a small part of an image to the sample size, or a tile requested past native zoom, comes out in blocks.  Items
 * (qoimi_resize as it is), modes (QOIMI_RESIZE_PLAIN, QOIMI_RESIZE_ALPHA_WEIGHTED), flips, outputs, staging, plan and the "not one byte beside an
 * output" contract are those of qoimi_decode_resized; only the weights differ.
 * The result (normative; qoi_amd/bilinear.py: bilinear states it in Python): D, R, cw, rh, ow, oh, och as for qoimi_decode_resized; all arithmetic
 * is integer, every division floors.  One axis, n_src source samples to n_out output samples, on a line of length 2 * n_src * n_out: source
 * sample k has its centre at (2k + 1) * n_out, output sample X at (2X + 1) * n_src; rad = 2 * max(n_src, n_out) - one source pitch when
 * enlarging, one output pitch when reducing; t(X, k) = max(0, rad - |(2X + 1) * n_src - (2k + 1) * n_out|) for 0 <= k < n_src;
 * W(X) = sum over k of t(X, k), at least 1.  Samples outside the rectangle do not exist: the weights are renormalised by W(X), not clamped.
 * tx, Wx come from (cw, ow), ty, Wy from (rh, oh).  Two axes, ONE rounding: D(X, Y) = Wx(X) * Wy(Y), N_c = sum over r, k of
 * ty(Y, r) * tx(X, k) * R[r][k].c.
 *   QOIMI_RESIZE_PLAIN           every channel of output pixel (X, Y) is (N_c + D/2) / D
 *   QOIMI_RESIZE_ALPHA_WEIGHTED  where och == 4: A = N_a, output alpha is (A + D/2) / D; if A > 0, r, g and b are (sum ty * tx * c * a + A/2) / A,
 *                                if A == 0 they are the PLAIN value.  With och == 3 this mode is PLAIN.
 * Flips and layout as for qoimi_decode_resized (the tent is symmetric: this is the resampled mirrored rectangle); ow * oh * och bytes
 * (qoimi_bilinear_size) at d_out + out_offsets[j].  With out_width x out_height equal to width x height there is a single sample of weight rad:
 * the call is qoimi_decode_crops byte for byte.  A constant rectangle gives the constant at any size.  When enlarging at most 2 x 2 samples have
 * a weight: the usual half-pixel-centre bilinear interpolation with replicated borders.  Against a float64 evaluation of the same filter
 * (torch.nn.functional.interpolate, mode "bilinear", antialias=True, align_corners=False) a value differs by at most 1, and only where the
 * float result lies at a rounding boundary.
 * Limits: width <= 32 * out_width and height <= 32 * out_height, so an output pixel has at most 64 x 64 source pixels with a weight; and
 * max(width, out_width) * max(height, out_height) < 2^30.  Then one weight ty * tx is below 2^32, D < 2^44, N_c < 2^52 and the alpha-weighted sums
 * are below 2^60.
 * Arguments, the plan (qoi_amd/bilinear.py: plan - that of qoimi_decode_crops over the items' rectangles), sub-batches and rejections are those
 * of qoimi_decode_resized, with two differences: QOIMI_E_ARG for width > 32 * out_width or height > 32 * out_height, and for
 * max(width, out_width) * max(height, out_height) >= 2^30.  Reported before anything is launched, the caller's buffers are untouched;
 * qoimi_last_error names the cause.  SYNCHRONOUS: returns when every output is written.  The sub-batches count as decode calls of the context.
 * One call at a time per context, as everywhere. */
int qoimi_decode_bilinear(qoimi_ctx *ctx, const void *d_streams, const size_t *stream_offsets /* host */, const int *sizes /* host */,
                          const qoi_desc *descs /* host */, int n_images, int channels /* 0, 3, 4 */,
                          const qoimi_resize *items /* host */, int n_items, int mode,
                          void *d_out, const size_t *out_offsets /* host, n_items */, size_t staging_bytes, void *stream);

/* out_width * out_height * channels - the bytes of the item's output - or 0 if desc is rejected, item is NULL, has a zero width or height in or
 * out, leaves the image of desc, reduces by more than 32 in an axis, reaches the product limit of 2^30 or carries an unknown flag bit, or
 * channels is not 3 / 4 (item->image is not looked at).  Pure host arithmetic: no context, no GPU. */
size_t qoimi_bilinear_size(const qoi_desc *desc, const qoimi_resize *item, int channels);

/* Of the context's last qoimi_decode_bilinear call: [0] sub-batches decoded, [1] launches of the filter kernel (it has no entry in
 * qoimi_kernel_name), [2] bytes of the staging the call planned for (its largest sub-batch), [3] images decoded (the referenced ones). */
void qoimi_bilinear_stats(qoimi_ctx *ctx, long long out[4]);

/* Rectangles of a pack's images sampled through an affine map, without the caller ever owning the decoded images: the calls above mirror a
 * rectangle but cannot turn the sampling grid - five of the eight EXIF orientations and every quarter turn of a tile need a transposition, and
 * rotation, shear and anisotropic scale about a point (the affine augmentation of a training loader, the rotated viewport of a slide or map
 * viewer) need a general map.  Channels, staging, plan, sub-batches and the "not one byte beside an output" contract are those of
 * qoimi_decode_resized; the modes are its QOIMI_RESIZE_PLAIN and QOIMI_RESIZE_ALPHA_WEIGHTED.
 * The result (normative; qoi_amd/warp.py: warp states it in Python): decode stream items[j].image exactly as qoimi_decode_images does (same
 * leniency, bit-exact for EVERY input stream) to och channels, which gives D; a 3-channel decode has alpha 255.  R = D[y .. y + height) x
 * [x .. x + width), cw = width, rh = height, ow = out_width, oh = out_height.  All arithmetic is integer, every shift and division floors.
 * Coordinates are DOUBLED pixel-centre coordinates with 16 fractional bits: the centre of source column k of R lies at (2k + 1) << 16.  Output
 * pixel (X, Y) has U = 2X + 1, V = 2Y + 1; the item carries the INVERSE map, from the output into R:
 *   Px = a * U + b * V + c,  Py = d * U + e * V + f       (the identity is a = e = 65536 with everything else 0)
 * Bilinear over 2 x 2 samples: px = Px - 65536, k0 = px >> 17 (arithmetic, so it floors for negatives), fx = px & 131071; columns k0 and
 * k0 + 1 have the weights 131072 - fx and fx; rows likewise from Py.  A sample with a weight of 0 counts as not taken.  Samples outside R are
 * never read, even where the image has pixels there: with QOIMI_WARP_REPLICATE their indices are clamped into R, otherwise they take `fill`
 * (bytes r, g, b, a little-endian; a 3-channel output ignores its alpha).  N_c = sum of wy * wx * c over the four samples.
 *   QOIMI_RESIZE_PLAIN           every channel of output pixel (X, Y) is (N_c + 2^33) >> 34: ONE rounding
 *   QOIMI_RESIZE_ALPHA_WEIGHTED  where och == 4: A = N_a, output alpha as in the plain mode; if A > 0, r, g and b are (sum wy * wx * c * a + A/2) / A,
 *                                if A == 0 they are the PLAIN value.  With och == 3 this mode is PLAIN.
 * The oh x ow result is written tightly packed row-major, ow * oh * och bytes (qoimi_warp_size), at d_out + out_offsets[j].
 * NO ANTIALIASING: a map that reduces still takes four samples per output pixel, as cv::warpAffine and torch's grid_sample do; reduce first with
 * qoimi_decode_resized or qoimi_decode_bilinear where that matters, or set QOIMI_WARP_SUPER2 / QOIMI_WARP_SUPER4 (below) for ratios up to 4 : 1.  With the identity the call is qoimi_decode_crops byte for byte; with
 * a = 65536 / s and REPLICATE it is qoimi_decode_bilinear enlarging by the power of two s; a constant rectangle stays the constant under any
 * map with REPLICATE.  Against a float64 evaluation of the same map (torch affine_grid + grid_sample, bilinear, align_corners=False) a value
 * differs by at most 1, and only where the float result lies at a rounding boundary.
 * QOIMI_WARP_NEAREST (a flag of the item, combinable with QOIMI_WARP_REPLICATE; normative; qoi_amd/warp.py: warp states it in Python) replaces
 * the 2 x 2 bilinear taps with ONE sample - selection, for label maps that take the geometry of their photograph: Px and Py are exactly as
 * above; column k = Px >> 17 and row r = Py >> 17 (arithmetic shifts: they floor for negative values); column k covers
 * [k << 17, (k + 1) << 17), with its centre at (2k + 1) << 16.  If k is outside [0, cw) or r is outside [0, rh): with REPLICATE the index is
 * clamped into R, without it the output pixel is `fill` (a 3-channel output ignores its alpha); samples outside R are never read.  The output
 * pixel is the sample, byte for byte, and both modes give the same bytes.  With the identity the call is qoimi_decode_crops; with any
 * qoimi_warp_orient item it equals the bilinear warp byte for byte, because every position is a pixel centre.  Limits, plan, staging and every
 * rejection are those of the bilinear warp; the flag rule reads: a bit other than QOIMI_WARP_REPLICATE and QOIMI_WARP_NEAREST (2 is not a
 * flag, nor is 8; QOIMI_WARP_BICUBIC, below, is the third flag).  The flag applies unchanged to qoimi_decode_warped_tensors and qoimi_decode_warped_indexed, and
 * qoimi_warp_size and qoimi_warp_tensor_size accept it.  Items with and without the flag mix freely in one call.
 * QOIMI_WARP_BICUBIC (a flag of the item, combinable with QOIMI_WARP_REPLICATE, never with QOIMI_WARP_NEAREST; normative; qoi_amd/warp.py: warp
 * states it in Python, qoi_amd/csrc/qoi_warp_cubic_core.h holds it in C++) replaces the 2 x 2 taps with 4 x 4 samples under Keys' cubic with
 * a = -1/2: the kernel of QOIMI_FILTER_BICUBIC and of PIL's BICUBIC, so both halves of the library give the same picture.  cv2.INTER_CUBIC and
 * torch's grid_sample(mode="bicubic") use a = -3/4 and therefore differ.  Px, Py, the limits and their order, the plan and the staging are
 * exactly those of the bilinear warp.  One axis, with u = 2^17: p = P - 65536, k0 = p >> 17 (arithmetic), fr = p & 131071; the four samples are
 * k0 - 1, k0, k0 + 1, k0 + 2 at the distances d = u + fr, fr, u - fr, 2u - fr, and c(d) is the formula of QOIMI_FILTER_BICUBIC:
 * 3d^3 - 5u d^2 + 2u^3 for d <= u, -d^3 + 5u d^2 - 8u^2 d + 4u^3 for u < d < 2u, 0 from 2u on (every term is below 2^56).  The four c add up to
 * W = 2u^3 = 2^52 for every fr.  q_j = (c_j + 2^36) >> 37 (arithmetic) - c_j * 2^15 / W rounded; the deficit 2^15 - sum q_j goes to the tap with
 * the largest c, the lowest j on a tie: the weights of an axis add up to exactly 2^15.  A tap with q == 0 counts as not taken and is never
 * read.  Samples outside R are never read, even where the image has pixels there: with QOIMI_WARP_REPLICATE each of the four indices is clamped
 * into R (the 64-bit index is tested before it is narrowed), without it the sample has the value `fill` and keeps its weight - there is no
 * renormalisation, as in the bilinear warp.  Two axes, one rounding: N_c = sum of qy * qx * c over the 4 x 4 samples.
 *   QOIMI_RESIZE_PLAIN           every channel is clamp((N_c + 2^29) >> 30, 0, 255): the negative lobes overshoot, the clamp is part of the definition
 *   QOIMI_RESIZE_ALPHA_WEIGHTED  where och == 4: A = N_a, alpha is the PLAIN value; if A > 0, r, g and b are clamp((sum qy * qx * c * a + A/2) / A, 0, 255)
 *                                with a flooring division; if A <= 0 - the negative lobes make that possible - they are the PLAIN value.  With
 *                                och == 3 this mode is PLAIN.
 * The |q| of an axis sum to at most 5 * 2^13 = 1.25 * 2^15 (at fr = u / 2 the weights are -1/16, 9/16, 9/16, -1/16), so a horizontal blend is
 * below 2^24 in magnitude, |N_c| < 2^40 and the alpha-weighted sums are below 2^48.
 * At a pixel centre, fr = 0 on both axes, the weights are (0, 2^15, 0, 0): the identity map gives qoimi_decode_crops byte for byte and every
 * qoimi_warp_orient item gives the bilinear warp byte for byte.  A constant rectangle stays the constant under any map with REPLICATE.  With
 * a = e = 65536 / s, s a power of two, b = c = d = f = 0 and an output of s times the rectangle, every output pixel whose 4 x 4 taps all lie
 * inside R equals QOIMI_FILTER_BICUBIC of qoimi_decode_tensors (U8, HWC) enlarging by s, byte for byte: the two definitions give the same
 * rational weights there and differ only at the border, where the filter renormalises and the warp replicates.  Against a float64 evaluation
 * of the same Keys kernel at the same positions with the same border rule, clamped and rounded, a PLAIN value differs by at most 1, and only
 * where the float result lies at a rounding boundary (qoi_amd/warp.py derives it from the quantisation of q, the deficit tap and the one
 * rounding: E < 0.036).  NO ANTIALIASING here either: a map that reduces takes sixteen samples.  The flag rule reads: a bit other than 1, 4 and
 * 16 is an unknown flag bit (2 and 8 are not flags); then QOIMI_WARP_NEAREST and QOIMI_WARP_BICUBIC together are rejected with a message of
 * their own.  The flag applies unchanged to qoimi_decode_warped_tensors and qoimi_decode_warped_indexed, and qoimi_warp_size and
 * qoimi_warp_tensor_size accept it.  Items with and without the flag mix freely in one call; a call with such an item runs a kernel of its own
 * that serves all its items, a call without one runs what it always ran.
 * QOIMI_WARP_REFLECT = 64, QOIMI_WARP_REFLECT_101 = 128 and QOIMI_WARP_WRAP = 256 (flags of the item; normative; qoi_amd/warp.py: warp and fold
 * state them in Python, qoi_amd/csrc/qoi_warp_border_core.h holds them in C++) are, with QOIMI_WARP_REPLICATE, THE BORDER: at most one of the
 * four may be set, and each of them combines with QOIMI_WARP_NEAREST or with QOIMI_WARP_BICUBIC.  Px, Py, k0, the fractions, the weights - the
 * bicubic deficit tap included -, the one rounding, the clamp, the alpha-weighted mode and the rule that a tap with the weight 0 is not taken
 * and never read stay exactly as they are for all three samplings: only the INDEX of a tap changes.  Every 64-bit tap index k on an axis of n
 * samples (n = cw for columns, rh for rows) is folded into [0, n) before anything is narrowed, and `fill` is not used, as with REPLICATE.
 * With `mod` the flooring modulo, 0 <= m < P for negative k too:
 *   QOIMI_WARP_REFLECT      "dcba|abcd|dcba" (numpy "symmetric", cv2.BORDER_REFLECT, torch grid_sample "reflection" with align_corners=False):
 *                           P = 2n, m = k mod P, the index is m < n ? m : P - 1 - m
 *   QOIMI_WARP_REFLECT_101  "dcb|abcd|cba" (numpy "reflect", cv2.BORDER_REFLECT_101 - the default of cv2.warpAffine pipelines and of
 *                           albumentations -, torchvision Pad "reflect"): if n == 1 the index is 0, else P = 2n - 2, m = k mod P, the index is
 *                           m < n ? m : P - m
 *   QOIMI_WARP_WRAP         "abcd|abcd|abcd" (numpy "wrap", cv2.BORDER_WRAP; panoramas, tiling textures): the index is k mod n
 * EACH TAP IS FOLDED ON ITS OWN - the 2 of the bilinear sampling, the 4 of the bicubic, the one of NEAREST - which is what cv2.warpAffine does
 * and, for REFLECT, equals torch's reflection of the coordinate.  The rectangle is still what is staged and what the border is taken at:
 * nothing outside R is ever read.  With the identity plus a whole-pixel translation into a larger output each border gives numpy.pad of R
 * with its mode, byte for byte, in all three samplings, for pads larger than n and for n == 1 too; a constant rectangle stays the constant;
 * every output pixel whose taps all lie inside R equals the call without the flag; against a float64 evaluation with the same border rule
 * the bounds of the bilinear and the bicubic warp hold unchanged (the arithmetic is theirs).  The flag rule reads, in this order: a bit other
 * than 1, 4, 16, 64, 128 and 256 is an unknown flag bit (2, 8 and 32 are not flags); QOIMI_WARP_NEAREST and QOIMI_WARP_BICUBIC together; more
 * than one of the four border flags, with a message of its own; reserved.  Limits, plan, staging and stats are untouched.  The flags apply
 * unchanged to qoimi_decode_warped_tensors and qoimi_decode_warped_indexed, and qoimi_warp_size and qoimi_warp_tensor_size accept them (0 for
 * two borders).  Items with and without a border flag, and of every sampling, mix freely in one call; a call with an item that carries one of
 * the three runs a kernel of its own that serves all its items, a call without one runs what it always ran.
 * QOIMI_WARP_SUPER2 = 1024 (s = 2, L = 1) and QOIMI_WARP_SUPER4 = 2048 (s = 4, L = 2) (flags of the item; normative; qoi_amd/warp.py: warp states
 * them in Python, qoi_amd/csrc/qoi_warp_super_core.h holds them in C++) SUPERSAMPLE a reducing map: an item carries at most one of the two,
 * with the bilinear sampling only; 512 is not a flag.  Everything about the item that is not named here stays as it is: R, cw, rh, U = 2X + 1,
 * V = 2Y + 1, the modes, the fill, the four borders, the plan, staging, limits, and the rule that a tap of weight 0 is not taken and never
 * read.  Output pixel (X, Y) is the mean of s x s bilinear samples laid on a regular grid inside the pixel, with ONE rounding.  For
 * 0 <= i, j < s:
 *   Us = s * U + 2i + 1 - s,   Vs = s * V + 2j + 1 - s        (the sub-sample's centre in coordinates s times finer)
 *   Px = ((a * Us + b * Vs) >> L) + c,   Py = ((d * Us + e * Vs) >> L) + f     (arithmetic shift: it floors)
 * From (Px, Py) the 2 x 2 taps, their weights (131072 - fx, fx and likewise for rows), their indices and the border are exactly those of the
 * bilinear warp today.  A tap outside R takes `fill`.  Under QOIMI_WARP_REPLICATE its index is clamped; under REFLECT / REFLECT_101 / WRAP it
 * is folded.  Each tap is treated on its own.  N_c = sum over all s^2 sub-samples and their four taps of wy * wx * c.
 *   QOIMI_RESIZE_PLAIN           every channel is (N_c + 2^(33 + 2L)) >> (34 + 2L)
 *   QOIMI_RESIZE_ALPHA_WEIGHTED  with och == 4: A = N_a, alpha is the PLAIN value.  If A > 0, r, g and b are (M_c + A / 2) / A, where M_c is the
 *                                same sum of wy * wx * c * a.  If A == 0 they are the PLAIN value.  With och == 3 this mode is PLAIN.
 * Bounds: Us, Vs < 2^23, so |a * Us + b * Vs| < 2^55; |Px|, |Py| < 2^57, as now, so the fold's preconditions hold unchanged;
 * N_c <= 255 * 2^38 < 2^46; M_c < 2^54.
 * With a = e = s * 65536, b = c = d = f = 0 and an output of (cw / s) x (rh / s), where s divides both, every sub-sample is a pixel centre.
 * The item is then the exact s x s box average with one rounding.  It equals qoimi_decode_thumbnails at factor s and qoimi_decode_resized of
 * the same rectangle byte for byte, in both modes: the rounding (S + cnt / 2) / cnt and the weighted (W + A / 2) / A of those calls come out
 * identical after the common factor 2^34 cancels.  A constant rectangle stays the constant under any map with any of the four borders.  The
 * result differs by at most 1 from a float64 evaluation of the same s^2 positions (taken from the integer Px, Py), bilinear, same border
 * rule, averaged and rounded once; it differs only where the float value lies at a rounding boundary, because N_c is exact.  There is NO
 * adaptivity: the flag takes s^2 sub-samples whether or not the map reduces.  Beyond 4 : 1 the result still aliases.
 * The flag rule reads, in this order: a bit other than 1, 4, 16, 64, 128, 256, 1024 and 2048 is an unknown flag bit (2, 8, 32 and 512 are not
 * flags); QOIMI_WARP_NEAREST and QOIMI_WARP_BICUBIC together; more than one of the four border flags; both SUPER flags together, with a message
 * of its own; a SUPER flag with QOIMI_WARP_NEAREST or QOIMI_WARP_BICUBIC, with a message of its own - supersampling is defined for the bilinear
 * sampling only; reserved != 0.  qoimi_warp_size and qoimi_warp_tensor_size accept the flags and return 0 for the two new rejections.  Items
 * with and without a SUPER flag, of every sampling and border, mix freely in one call; a call with a SUPER item runs a kernel of its own that
 * serves all its items, a call without one launches exactly what it launches today.  The flags apply unchanged to
 * qoimi_decode_warped_tensors and qoimi_decode_warped_indexed.
 * QOIMI_WARP_VOTE2 = 8192 (s = 2, L = 1) and QOIMI_WARP_VOTE4 = 16384 (s = 4, L = 2) (flags of the item; normative; qoi_amd/warp.py: warp states
 * them in Python, qoi_amd/csrc/qoi_warp_vote_core.h holds them in C++) take a MAJORITY VOTE under a reducing map, for label maps
 * (segmentation masks, instance ids, palette indices), where QOIMI_WARP_NEAREST looks at one source pixel per output pixel and thin classes
 * come and go with the sampling phase.  The flags are a fourth sampling: an item carries at most one of the two; neither combines with
 * QOIMI_WARP_NEAREST, QOIMI_WARP_BICUBIC, QOIMI_WARP_SUPER2 or QOIMI_WARP_SUPER4; either combines with the fill (no border flag) or with any
 * one of the four borders; 4096 is not a flag.  Everything about the item that is not named here stays as it is: R, cw, rh, U = 2X + 1,
 * V = 2Y + 1, limits and their order, plan, staging, stats, tiles.  Output pixel (X, Y) is the majority vote of s x s nearest sub-samples
 * on the grid QOIMI_WARP_SUPER2 / QOIMI_WARP_SUPER4 lays inside the pixel: for 0 <= i, j < s, Us, Vs, Px and Py are exactly those above,
 * with the arithmetic shift and the bounds |Px|, |Py| < 2^57.  The value of a sub-sample is that of QOIMI_WARP_NEAREST at (Px, Py): column
 * k = Px >> 17, row r = Py >> 17, the 64-bit index tested before it is narrowed; inside R it is R[r][k], all four bytes of the 4-channel
 * decode (a 3-channel stream has alpha 255).  Outside R each index is clamped under QOIMI_WARP_REPLICATE; under QOIMI_WARP_REFLECT,
 * QOIMI_WARP_REFLECT_101 or QOIMI_WARP_WRAP each index is folded on its own; without a border flag the value is the dword `fill` as given,
 * all four bytes, and nothing is read.  Nothing outside R is ever read.
 * The vote: a value votes as a whole dword.  The count of a value is the number of the s^2 sub-samples equal to it; the winners are the
 * values with the largest count.  One winner is the output; of several winners the output is the centre value if it is a winner, otherwise
 * the winner with the lowest key r << 24 | g << 16 | b << 8 | a - the vote and the tie rule of QOIMI_FILTER_MODE.  The centre value is what
 * QOIMI_WARP_NEAREST gives this output pixel with the same border or fill, from Px = a * U + b * V + c, Py = d * U + e * V + f; it does not
 * vote, and like any sub-sample it is the dword `fill`, with nothing read, where its position lies outside R and no border flag is set.
 * Both modes give the same bytes; och 3 drops alpha after the vote.
 * Consequences.  No invented value: every output pixel is one of its sub-sample values.  Identity and orientations: with the identity map,
 * and with every qoimi_warp_orient item, all s^2 sub-samples fall into the pixel the centre falls into (the offsets are at most 49152 < 65536
 * from a pixel centre, and a * Us is a multiple of 2^L), so the item is qoimi_decode_crops, respectively the QOIMI_WARP_NEAREST warp, byte
 * for byte.  Whole-factor reduction: with a = e = s * 65536, b = c = d = f = 0 and an output of (cw / s) x (rh / s), where s divides both,
 * sub-sample (i, j) is the centre of source pixel (sX + i, sY + j) and the centre value is pixel (sX + s/2, sY + s/2); the item then equals
 * QOIMI_FILTER_MODE of qoimi_decode_tensors (U8, HWC) for that rectangle and size and QOIMI_TILE_MODE at factor s, byte for byte, in both
 * modes and both channel counts.  A constant rectangle stays the constant under any map with any of the four borders.  There is NO
 * adaptivity: the flag takes s^2 sub-samples and the centre whether or not the map reduces, and beyond 4 : 1 the result still skips pixels.
 * The flag rule reads, in this order: a bit other than 1, 4, 16, 64, 128, 256, 1024, 2048, 8192 and 16384 is an unknown flag bit (2, 8, 32,
 * 512 and 4096 are not flags); QOIMI_WARP_NEAREST and QOIMI_WARP_BICUBIC together; more than one of the four border flags; both SUPER flags
 * together; a SUPER flag with QOIMI_WARP_NEAREST or QOIMI_WARP_BICUBIC; both VOTE flags together, with a message of its own; a VOTE flag with
 * QOIMI_WARP_NEAREST, QOIMI_WARP_BICUBIC, QOIMI_WARP_SUPER2 or QOIMI_WARP_SUPER4, with a message of its own - the vote is a sampling of its
 * own; reserved != 0.  qoimi_warp_size and qoimi_warp_tensor_size accept the flags and return 0 for the two new rejections.  Items with and
 * without a VOTE flag, of every sampling and border, mix freely in one call; a call with a VOTE item runs a kernel of its own that serves
 * all its items, a call without one launches exactly what it launches today.  The flags apply unchanged to qoimi_decode_warped_tensors and
 * qoimi_decode_warped_indexed: QOIMI_TENSOR_I64 with QOIMI_TENSOR_HW is the N x H x W a loss function takes.
 * Not here (of the vote): votes over more than 4 x 4 sub-samples, weighted or per-channel votes, adaptive sub-sample counts.
 * QOIMI_WARP_PROJECTIVE = 131072 (1 << 17) (a flag of the item; normative; qoi_amd/warp.py: positions states it in Python,
 * qoi_amd/csrc/qoi_warp_proj_core.h holds it in C++) makes the map a PERSPECTIVE map - a homography of the output rectangle: RandomPerspective
 * and the homography augmentations of a training loader, a tilted viewport, a document rectified from a photograph.  32768 and 65536 are not
 * flags.  The flag combines with the fill (no border flag) or any one of the four borders and with the bilinear sampling, QOIMI_WARP_NEAREST
 * or QOIMI_WARP_BICUBIC; it never combines with QOIMI_WARP_SUPER2, QOIMI_WARP_SUPER4, QOIMI_WARP_VOTE2 or QOIMI_WARP_VOTE4.  With the flag set
 * `reserved` is not 0: it holds the two perspective coefficients g = (int16)(reserved & 0xFFFF) and h = (int16)(reserved >> 16), both two's
 * complement; without the flag reserved != 0 is rejected exactly as before.  All arithmetic is integer, every division and shift floors;
 * ow = out_width, oh = out_height:
 *   L = the smallest integer >= 0 with 2^L >= max(ow, oh);  F = 14 + L, so F is 14..34
 *   U = 2X + 1, V = 2Y + 1 as above;  Uc = U - ow, Vc = V - oh: the doubled offsets from the output's centre, |Uc| < ow, |Vc| < oh
 *   Nx = a * U + b * V + c,  Ny = d * U + e * V + f: the Px and Py of an item without the flag
 *   W  = 2^F + g * Uc + h * Vc: the denominator is 1.0 at the centre of the output
 *   Px = floor(Nx * 2^F / W),  Py = floor(Ny * 2^F / W)
 * From Px and Py on nothing changes: k0, the fractions and the weights; the NEAREST column Px >> 17; the cubic weights; the clamp or fold of
 * each tap on its own; the fill; both alpha modes and the one rounding; the byte and tensor stores.  The scale is sized by the item: W > 0
 * everywhere requires |gamma| * ow < 1 for the real coefficient gamma, so the useful range of g is 1 / ow; a fixed scale would waste bits on
 * small outputs and lose sub-pixel accuracy on large ones, and with F = 14 + L the 16 bits cover exactly that range at every size.
 * Limits of an item with the flag, checked behind all the limits below, in this order, each with a message of its own: the flag together
 * with a SUPER or VOTE flag; |c| or |f| of 2^53 or more; 2^F - |g| * (ow - 1) - |h| * (oh - 1) < 2^(F - 3) - W is linear, so this is its
 * exact minimum over the pixel grid, and the limit keeps the denominator at or above 1/8 inside the output.  Then |Nx| < 2^52 + 2^52 + 2^53 =
 * 2^54, 2^(F-3) <= W < 5 * 2^F < 2^37 and |Px| <= 8 * |Nx| < 2^57, the bound of an item without the flag.  qoimi_warp_size and
 * qoimi_warp_tensor_size accept the flag and return 0 for the three new rejections.
 * Consequences.  With g = h = 0, W = 2^F and Px = Nx: the item gives the bytes of the same item without the flag, in every sampling, border,
 * mode and format.  The map applied is the QUANTISED homography, exactly - still a homography, so lines stay lines; qoi_amd/warp.py:
 * homography and perspective quantise a 3 x 3 matrix or four corner points and REPORT the displacement that costs at the output's corners
 * (it is not promised).  Against a float64 evaluation of that same quantised map a bilinear value differs by at most 1, and only at a
 * rounding boundary: the position is floored by less than 2^-17 of a pixel.  A constant rectangle stays the constant under
 * QOIMI_WARP_REPLICATE.  Items with and without the flag, of every sampling and border, SUPER and VOTE items included, mix freely in one
 * call; a call with a projective item runs a kernel of its own that serves all its items, a call without one launches exactly what it
 * launches today.  The flag applies unchanged to qoimi_decode_warped_tensors and qoimi_decode_warped_indexed.
 * Not here (of the projective map): projective SUPER and VOTE items, a free denominator at the origin (the map is normalised at the centre
 * of the output), coefficients wider than 16 bits, W <= 0 - a horizon inside the output.
 * Not here: other cubic kernels (a = -3/4), Lanczos in the warp, adaptive antialiasing of reducing maps, supersampling beyond 4 x 4,
 * supersampled bicubic or nearest, projective maps with a supersampling or a vote, a border per axis, mixing reflect with a fill.
 * The rectangle is what is staged and what the border is taken at: rows_i of the plan is the maximum of y + height over the items of image i,
 * so the caller keeps the rectangle tight around what the map reaches - a rectangle of the whole image under a map that reaches one corner
 * decodes the whole image.
 * Limits, checked per item in this order: a zero width, height, out_width or out_height; a rectangle that leaves its image; out_width or
 * out_height of 2^20 or more; out_width * out_height of 400 000 000 or more; |c| or |f| of 2^56 or more; a flag bit other than
 * QOIMI_WARP_REPLICATE, QOIMI_WARP_NEAREST, QOIMI_WARP_BICUBIC, QOIMI_WARP_REFLECT, QOIMI_WARP_REFLECT_101 and QOIMI_WARP_WRAP, then NEAREST and
 * BICUBIC together, then more than one of the four border flags (QOIMI_WARP_SUPER2 and QOIMI_WARP_SUPER4 are flags too; then both of them
 * together, then one of them with NEAREST or BICUBIC; QOIMI_WARP_VOTE2 and QOIMI_WARP_VOTE4 likewise; then both of them together, then one
 * of them with NEAREST, BICUBIC or a SUPER flag; QOIMI_WARP_PROJECTIVE is a flag too); reserved != 0 without QOIMI_WARP_PROJECTIVE, with it the three limits named there.  Then U, V < 2^21, |a * U| and |b * V| are at most 2^31 * 2^21 = 2^52, and |Px|, |Py| < 2^56 + 2 * 2^52 <
 * 2^57: both positions fit 64 bits with room to spare.  N_c <= 255 * 2^34 < 2^42, the alpha-weighted sums are below 2^50.
 *   stream_offsets, sizes, descs, channels, out_offsets, staging_bytes  as for qoimi_decode_resized; the plan is that of qoimi_decode_crops
 *                  over the items' rectangles (normative; qoi_amd/warp.py: plan)
 *   items          HOST qoimi_warp[n_items], in any order of image; several may name the same image, their rectangles may overlap or coincide
 * Every sub-batch is one qoimi_decode_images call as it is, at 4 output channels and with each descriptor's height replaced by rows_i, then one
 * launch of the warp kernel over all items of the sub-batch's images on `stream`.
 * SYNCHRONOUS: returns when every output is written.  QOIMI_E_ARG for what qoimi_decode_resized rejects (its ratio limit and flag bits apart),
 * for the limits above, and for a sub-batch of the plan with 2^31 - 1 or more tiles of 16 x 16 output pixels: reported before anything is
 * launched, the caller's buffers are untouched; qoimi_last_error names the cause.  Output ranges must not overlap.  The sub-batches count as
 * decode calls of the context.  One call at a time per context, as everywhere. */
enum { QOIMI_WARP_REPLICATE = 1, QOIMI_WARP_NEAREST = 4, QOIMI_WARP_BICUBIC = 16,      /* 2, 8 and 32 are not flags */
       QOIMI_WARP_REFLECT = 64, QOIMI_WARP_REFLECT_101 = 128, QOIMI_WARP_WRAP = 256,    /* at most one of these three and REPLICATE */
       QOIMI_WARP_SUPER2 = 1024, QOIMI_WARP_SUPER4 = 2048,                              /* at most one; bilinear only; 512 is not a flag */
       QOIMI_WARP_VOTE2 = 8192, QOIMI_WARP_VOTE4 = 16384,                               /* at most one; a sampling of its own; 4096 is not a flag */
       QOIMI_WARP_PROJECTIVE = 131072 };                                                /* reserved holds g and h; never with SUPER or VOTE; 32768 and 65536 are not flags */
typedef struct {                 /* 72 bytes, offsets 0/4/8/12/16/20/24/28/32/36/40/44/48/52/56/64 */
    unsigned int image;          /* index into the call's images */
    unsigned int x, y;           /* top-left corner of the source rectangle */
    unsigned int width, height;  /* both >= 1; x + width <= image width, y + height <= image height */
    unsigned int out_width, out_height;  /* both >= 1 and below 2^20; their product below 400 000 000 */
    unsigned int flags;          /* one border at most (REPLICATE, REFLECT, REFLECT_101, WRAP), QOIMI_WARP_NEAREST or QOIMI_WARP_BICUBIC, or QOIMI_WARP_SUPER2 or QOIMI_WARP_SUPER4, or QOIMI_WARP_VOTE2 or QOIMI_WARP_VOTE4; QOIMI_WARP_PROJECTIVE with none of the last four; no other bit */
    int a, b, d, e;              /* the linear part of the inverse map, 16 fractional bits */
    unsigned int fill;           /* r | g << 8 | b << 16 | a << 24: the value of a sample outside the rectangle without a border flag */
    unsigned int reserved;       /* 0; with QOIMI_WARP_PROJECTIVE g = (int16)(reserved & 0xFFFF) and h = (int16)(reserved >> 16) */
    long long c, f;              /* the offsets of the inverse map, doubled coordinates with 16 fractional bits; |c|, |f| < 2^56, with QOIMI_WARP_PROJECTIVE < 2^53 */
} qoimi_warp;
int qoimi_decode_warped(qoimi_ctx *ctx, const void *d_streams, const size_t *stream_offsets /* host */, const int *sizes /* host */,
                        const qoi_desc *descs /* host */, int n_images, int channels /* 0, 3, 4 */,
                        const qoimi_warp *items /* host */, int n_items, int mode,
                        void *d_out, const size_t *out_offsets /* host, n_items */, size_t staging_bytes, void *stream);

/* out_width * out_height * channels - the bytes of the item's output - or 0 if desc is rejected, item is NULL or breaks one of the limits of
 * qoimi_decode_warped, or channels is not 3 / 4 (item->image is not looked at).  Pure host arithmetic: no context, no GPU. */
size_t qoimi_warp_size(const qoi_desc *desc, const qoimi_warp *item, int channels);

/* Of the context's last qoimi_decode_warped call: [0] sub-batches decoded, [1] launches of the warp kernel (it has no entry in
 * qoimi_kernel_name), [2] bytes of the staging the call planned for (its largest sub-batch), [3] images decoded (the referenced ones). */
void qoimi_warp_stats(qoimi_ctx *ctx, long long out[4]);

/* Fills *out with the item that shows the rectangle (x, y, width, height) of an image of desc in the EXIF orientation 1..8, exactly: every
 * output pixel is one pixel of the rectangle (1 as it is, 2 mirrored left-right, 3 turned by 180 degrees, 4 mirrored top-bottom, 5 transposed,
 * 6 turned by 90 degrees clockwise, 7 transposed along the other diagonal, 8 turned by 90 degrees counter-clockwise).  out_width x out_height is
 * width x height, height x width for 5..8; image, flags, fill and reserved are 0: the caller sets image.  0 on success; QOIMI_E_ARG for a NULL or
 * rejected desc, a NULL out, an orientation outside 1..8, a zero width or height, a rectangle that leaves the image.  Pure host arithmetic. */
int qoimi_warp_orient(const qoi_desc *desc, unsigned x, unsigned y, unsigned width, unsigned height, int exif_orientation /* 1..8 */,
                      qoimi_warp *out);

/* The outputs of qoimi_decode_resized, qoimi_decode_bilinear and qoimi_decode_warped as TENSORS: what a training loader feeds a model is not
 * 8-bit interleaved pixels but N x C x H x W (or N x H x W x C) in binary32, binary16 or bfloat16, each channel normalised -
 * (p / 255 - mean) / std is scale = 1 / (255 * std), bias = -mean / std.  The conversion happens where the filter's rounded pixel still is in a
 * register: no second kernel of the caller's reads the bytes back, and nothing but the tensor is written.  Items (qoimi_resize, qoimi_warp as
 * they are), channels, modes, flips, border, staging, plan, sub-batches, the tile limits and the "not one byte beside an output" contract are
 * those of the underlying call: qoimi_decode_resized for QOIMI_FILTER_AREA, qoimi_decode_bilinear for QOIMI_FILTER_BILINEAR, qoimi_decode_warped
 * for qoimi_decode_warped_tensors.  QOIMI_FILTER_BICUBIC has no call of its own - its "underlying call" is the definition below, everything
 * but the filter and its limits as for qoimi_decode_bilinear; QOIMI_TENSOR_U8 with QOIMI_TENSOR_HWC gives its plain interleaved bytes.
 * QOIMI_FILTER_LANCZOS and QOIMI_FILTER_NEAREST likewise, and QOIMI_FILTER_MODE.
 * The result (normative; qoi_amd/tensors.py: convert states it in Python): let P be the oh x ow x och u8 result of the underlying call with the
 * same items, channels and mode, byte for byte, flips included.  Element (Y, X, c) of output j has the value v = P[Y][X][c], an integer 0..255.
 *   QOIMI_TENSOR_U8    the element is v; scale must be all 1.0f and bias all +0.0f
 *   QOIMI_TENSOR_F32   t = (float)v; m = t * scale[c], rounded to nearest even in binary32; s = m + bias[c], rounded to nearest even in
 *                      binary32: TWO roundings, never a fused multiply-add; the element is s
 *   QOIMI_TENSOR_F16, QOIMI_TENSOR_BF16   s converted to binary16 / bfloat16, round to nearest even
 *   QOIMI_TENSOR_I32, QOIMI_TENSOR_I64   the element is v as a little-endian two's-complement integer of 4 / 8 bytes - the integer class-index dtypes
 *                      a loss function takes; scale must be all 1.0f and bias all +0.0f, as for QOIMI_TENSOR_U8
 * Subnormals are kept, not flushed, in every format; a result too large for its format becomes infinity.  scale and bias are per channel r, g,
 * b, a; a 3-channel output ignores the fourth.  The element is stored at element index (Y * ow + X) * och + c for QOIMI_TENSOR_HWC, at
 * (c * oh + Y) * ow + X for QOIMI_TENSOR_CHW, from d_out + out_offsets[j]; an output is tightly packed, ow * oh * och * element size bytes
 * (qoimi_tensor_size, qoimi_warp_tensor_size).  With QOIMI_TENSOR_HW only the FIRST channel (r) of each pixel is stored, as one plane: element
 * index Y * ow + X, scale[0] and bias[0] (the others are ignored but must still be finite), an output of ow * oh * element size bytes - the
 * sizes, the overlap check and the alignment check count it that way; `channels` still says how the image is decoded, the layout only chooses
 * what is stored.  Every layout goes with every dtype, every filter and the warp: QOIMI_TENSOR_I64 with QOIMI_TENSOR_HW is the N x H x W of
 * class indices a loss function takes.  QOIMI_TENSOR_U8 with QOIMI_TENSOR_HWC therefore is the underlying call byte for byte, and every
 * other format a pure function of its bytes: the exact-integer definitions of the three filters stand as they are.
 * QOIMI_TENSOR_HW_ID24 is one plane, as QOIMI_TENSOR_HW is: the element at index Y * ow + X is r | g << 8 | b << 16 of the pixel the u8
 * call would store at (Y, X) - the 24-bit id of the COCO panoptic convention id = R + 256 * G + 256^2 * B, what QOIMI_TILE_LABELS_ID24
 * packs and what a panoptic PNG converted to QOI holds.  Alpha is ignored (channels 3 and 4 give the same ids); `channels` still only says
 * how the image is decoded; sizes, overlap and alignment count one element per pixel.  It goes with QOIMI_TENSOR_I32 and QOIMI_TENSOR_I64
 * only, whose scale is 1 and bias +0.  It goes with every filter and the warp, the element being a pure function of the underlying
 * call's bytes, but it MEANS something only under the selections, which invent no pixel: QOIMI_FILTER_NEAREST / _MODE and
 * QOIMI_WARP_NEAREST / _VOTE2 / _VOTE4; an averaged id is no id.
 * Only whole, naturally aligned elements are stored (u8 HWC: as the underlying call stores): no word is read and written back, two outputs
 * may share one.
 * QOIMI_FILTER_BICUBIC (normative; qoi_amd/bicubic.py: bicubic states it in Python) is the antialiased bicubic filter - Keys' cubic with
 * a = -1/2, stretched by the reduction factor when reducing: PIL BICUBIC, torchvision Resize(BICUBIC, antialias=True).  D, R, cw, rh, ow, oh,
 * och, the items, flips, modes and the plan as for qoimi_decode_bilinear; all arithmetic is integer, every division and every shift floors,
 * for negative numbers too.  One axis, n_src source samples to n_out output samples, on the line of the tent filter: source sample k has its
 * centre at (2k + 1) * n_out, output sample X at (2X + 1) * n_src; u = 2 * max(n_src, n_out); for 0 <= k < n_src,
 * d = |(2X + 1) * n_src - (2k + 1) * n_out| and
 *   c(X, k) = 3d^3 - 5u d^2 + 2u^3               for d <= u
 *   c(X, k) = -d^3 + 5u d^2 - 8u^2 d + 4u^3      for u < d < 2u    (negative)
 *   c(X, k) = 0                                  from 2u on
 * - 2u^3 times Keys' kernel at d / u.  W(X) = sum_k c(X, k) > 0: samples outside the rectangle do not exist, the weights are renormalised,
 * not clamped.  q(X, k) = (c(X, k) * 2^15 + W / 2) / W; the deficit 2^15 - sum_k q(X, k) is added to the tap with the largest c, the lowest
 * such k on a tie, so sum_k q(X, k) = 2^15 for every X.  qx from (cw, ow), qy from (rh, oh); two axes, ONE rounding:
 * N_c = sum_{r,k} qy(Y, r) * qx(X, k) * R[r][k].c.
 *   QOIMI_RESIZE_PLAIN            every channel is clamp((N_c + 2^29) >> 30, 0, 255)
 *   QOIMI_RESIZE_ALPHA_WEIGHTED   och == 4: A = N_a; alpha is the PLAIN value; where A > 0 r, g and b are
 *                                 clamp((sum qy*qx*c*a + A / 2) / A, 0, 255), where A <= 0 the PLAIN value.  och == 3: PLAIN
 * The clamp is part of the definition: the negative lobes overshoot at edges.  The flips are those of the tent filter (the kernel is
 * symmetric).  With out_width x out_height equal to width x height the only tap with c != 0 is k = X, q = 2^15: the rectangle byte for
 * byte; a constant rectangle gives the constant at any size; enlarging touches at most 4 x 4 samples.  Against a float64 evaluation of the
 * same renormalised filter, rounded and clamped, a PLAIN value differs by at most 1 for every geometry accepted (qoi_amd/bicubic.py derives
 * it from the quantisation of q, the deficit tap and the one rounding: below 1.24 from the exact real value with 64 taps in both axes).
 * Its limits, each a QOIMI_E_ARG item by item where the other filters have their ratio limit: width <= 16 * out_width and
 * height <= 16 * out_height (at most 64 taps per axis); max(width, out_width) <= 16384 and max(height, out_height) <= 16384 (|c| <= 2^46,
 * W < 2^52, |N_c| < 2^40, the alpha-weighted sums below 2^48: signed 64 bits hold everything).
 * QOIMI_FILTER_LANCZOS (normative; qoi_amd/lanczos.py: lanczos states it in Python) is the antialiased Lanczos filter with three lobes -
 * sinc(t) * sinc(t / 3) for |t| < 3, stretched by the reduction factor when reducing: PIL's Image.LANCZOS.  Everything as for
 * QOIMI_FILTER_BICUBIC - the line, the centres, u, d, W, q with its deficit tap, two axes with ONE rounding, both modes, the clamp, the flips -
 * but c.  The kernel table: T[i] = round(2^30 * sinc(i / 1024) * sinc(i / 3072)) for i = 0 .. 3072, sinc(t) = sin(pi t) / (pi t),
 * T[0] = 2^30, T[3072] = 0 - 3073 numbers that are data (qoi_amd/csrc/qoi_lanczos_table.h holds them; T[512] = 652756755,
 * T[1536] = -145057057, the smallest is -158126265).  c(X, k) = 0 for d >= 3u; else with z = 1024 * d, i = z / u, r = z - i * u,
 *   c(X, k) = T[i] * (u - r) + T[i + 1] * r
 * - u times the table interpolated linearly.  W(X) > 0 is asserted by the model over the geometries it walks, not proven.  With out_width x
 * out_height equal to width x height the only tap is k = X: the rectangle byte for byte; a constant rectangle gives the constant at any
 * size; enlarging touches at most 6 x 6 samples.  Against a float64 evaluation of the same renormalised filter from sinc, rounded and
 * clamped, a PLAIN value differs by at most 1 where the taps of the two axes, each less one, add up to 125 or less, and by at most 2 up to
 * the limits (qoi_amd/lanczos.py derives it from the quantisation of q, the deficit tap, the table's interpolation and the one rounding;
 * the largest difference the tests see is 1).  PIL rounds between its two passes and differs from this by a few units.
 * Its limits are those of QOIMI_FILTER_BICUBIC, each a QOIMI_E_ARG item by item: width <= 16 * out_width and height <= 16 * out_height (at
 * most 96 taps per axis); max(width, out_width) <= 16384 and max(height, out_height) <= 16384.
 * QOIMI_FILTER_NEAREST (normative; qoi_amd/nearest.py: nearest states it in Python) is selection, not a filter that averages - for label
 * maps: segmentation masks, instance ids, palette indices, whose values must not be mixed.  D, R, cw, rh, ow, oh and och as for
 * qoimi_decode_resized; all arithmetic is integer and floors.  Output pixel (X, Y) is R[r][k] byte for byte, with
 *   k = ((2X + 1) * cw) / (2 * ow),  r = ((2Y + 1) * rh) / (2 * oh)
 * - the source pixel whose cell holds the output pixel's centre, on the line the tent filter uses (a centre on the boundary of two cells
 * belongs to the upper one).  k < cw always holds: nothing outside R is read.  Both modes give the same bytes of it; a 3-channel decode has
 * alpha 255, och 3 drops alpha.  QOIMI_RESIZE_FLIP_X / _Y reverse the columns / rows of that result.  With the output the size of the rectangle
 * it is qoimi_decode_crops; with cw = f * ow it takes column X * f + f / 2; and it equals qoimi_decode_warped with QOIMI_WARP_NEAREST and the map
 * a = 65536 * cw / ow, e = 65536 * rh / oh, everything else 0, wherever both quotients are whole.  torch's interpolate(mode="nearest-exact")
 * computes the same index in float and is one lower at some of the positions where (2X + 1) * cw is a multiple of 2 * ow; there the integer
 * definition is the exact one.
 * Its limits, each a QOIMI_E_ARG item by item, in this order: the rectangle rules of the other filters (a zero size, an unknown flag bit, a
 * rectangle that leaves its image); then max(width, out_width) <= 16384 and max(height, out_height) <= 16384 - the size limit of
 * QOIMI_FILTER_BICUBIC ((2X + 1) * cw < 2^29: no 64-bit division).  There is NO ratio limit: every output pixel is one load.
 * QOIMI_FILTER_MODE (normative; qoi_amd/mode.py: mode states it in Python) is a majority vote - for REDUCING label maps, where
 * QOIMI_FILTER_NEAREST looks at one pixel of each cell and thin classes come and go with the sampling phase.  D, R, cw, rh, ow, oh and och
 * as for qoimi_decode_resized; the image is decoded to 4 channels, a 3-channel stream has alpha 255; all arithmetic is integer and floors.
 * On an axis of n_src source and n_out output samples the cell of output sample Z is [first(Z), first(Z + 1)) with
 *   first(Z) = (2 * Z * n_src + n_out - 1) / (2 * n_out)
 * - the source samples whose centre lies in the output sample's extent, on the line QOIMI_FILTER_NEAREST uses.  An empty cell (only when
 * enlarging on that axis) is replaced by the single sample ((2Z + 1) * n_src) / (2 * n_out), the nearest one.  The non-empty cells of an axis
 * partition [0, n_src) in order; the nearest sample lies in every non-empty cell.  Output pixel (X, Y) looks at the pixels of R in columns
 * cell(X) x rows cell(Y), at most 16 x 16 of them.  A pixel votes as a whole, all four bytes as decoded: colour-coded masks and 24-bit
 * instance ids survive, no colour is invented.  The count of a value is the number of pixels equal to it; the winners are the values with the
 * largest count.  One winner is the output.  Of several winners the output is the pixel QOIMI_FILTER_NEAREST would take - R[r][k] with
 * that filter's k and r - if it is a winner, else the winner with the lowest key = r << 24 | g << 16 | b << 8 | a.  (At 2 : 1 every straight
 * class boundary makes 2-2 ties; the lowest key alone would grow class 0 along each of them.)  Both modes give the same bytes; och 3 drops
 * alpha after the vote (two colours of a 4-channel stream that differ in alpha alone vote apart); QOIMI_RESIZE_FLIP_X / _Y reverse the columns / rows of that result.  With the output the size of the rectangle or larger on both axes
 * it is QOIMI_FILTER_NEAREST byte for byte; an image whose pixels are all distinct gives QOIMI_FILTER_NEAREST at any size; a constant
 * rectangle gives the constant; with cw = f * ow and rh = g * oh the cells are the f x g blocks.
 * Its limits, each a QOIMI_E_ARG item by item, in this order: the rectangle rules of the other filters; then width <= 16 * out_width and
 * height <= 16 * out_height (a cell is at most 16 x 16 pixels); then max(width, out_width) <= 16384 and max(height, out_height) <= 16384
 * (2 * Z * n_src + n_out < 2^30: no 64-bit division).
 *   filter         QOIMI_FILTER_LANCZOS, QOIMI_FILTER_AREA, QOIMI_FILTER_BILINEAR or QOIMI_FILTER_BICUBIC, or QOIMI_FILTER_NEAREST
 *                  or QOIMI_FILTER_MODE (qoimi_decode_tensors only)
 *   format         HOST; one for the whole call
 *   d_out, out_offsets   every d_out + out_offsets[j] a multiple of the element size (1 / 2 / 2 / 4, 4 / 8 for QOIMI_TENSOR_I32 / _I64)
 *   everything else      as for the underlying call
 * SYNCHRONOUS: returns when every output is written.  QOIMI_E_ARG, looked for in this order: an unknown filter; a NULL or empty argument
 * (format apart); channels; mode; the format - NULL, an unknown dtype, an unknown layout, reserved != 0, a scale or bias that is not finite,
 * QOIMI_TENSOR_U8, QOIMI_TENSOR_I32 or QOIMI_TENSOR_I64 with a scale other than 1 or a bias other than +0, QOIMI_TENSOR_HW_ID24 with a dtype other than QOIMI_TENSOR_I32 / _I64 (the last of the format checks; its message names ID24); then everything the underlying call rejects, with its messages, item by
 * item - an output whose size in BYTES does not fit a size_t or that ends behind the address space among them -, output ranges that overlap,
 * in bytes; an output address that is not a multiple of the element size; a sub-batch of the plan with 2^31 - 1 tiles or more.  All are
 * reported before anything is launched, the caller's buffers are untouched; qoimi_last_error names the cause.  The sub-batches count as decode
 * calls of the context.  One call at a time per context, as everywhere.
 * Not here: indexed forms, a majority (mode) filter per channel, with weights or over cells above 16 x 16 (QOIMI_FILTER_MODE votes on whole
 * pixels of cells up to that; the warp has QOIMI_WARP_VOTE2 / QOIMI_WARP_VOTE4), 16-bit or signed label sources (a label is a byte of the image, or with QOIMI_TENSOR_HW_ID24 three), ids above 2^24 - 1, a remapping table from byte to class index, a single
 * 8-byte store per QOIMI_TENSOR_I64 element (it is two dword stores), a u8 entry point or a stats function of the bicubic, the Lanczos, the nearest or the mode filter's own, other cubic kernels (a = -3/4), other Lanczos windows, a format per item, tensor forms of qoimi_decode_thumbnails and qoimi_decode_crops (an item whose output has the
 * size of its rectangle, or divides it, is those). */
enum { QOIMI_TENSOR_U8 = 0, QOIMI_TENSOR_F16 = 1, QOIMI_TENSOR_BF16 = 2, QOIMI_TENSOR_F32 = 3 };   /* element sizes 1 / 2 / 2 / 4 */
enum { QOIMI_TENSOR_I32 = 5, QOIMI_TENSOR_I64 = 6 };   /* element sizes 4 / 8; 4 is not a dtype */
enum { QOIMI_TENSOR_HWC = 0, QOIMI_TENSOR_CHW = 1, QOIMI_TENSOR_HW = 3 };   /* 2 is not a layout */
enum { QOIMI_TENSOR_HW_ID24 = 5 };   /* one plane of r | g << 8 | b << 16, QOIMI_TENSOR_I32 / _I64 only; 4 is not a layout */
enum { QOIMI_FILTER_AREA = 0, QOIMI_FILTER_BILINEAR = 1, QOIMI_FILTER_BICUBIC = 3, QOIMI_FILTER_LANCZOS = 6 };   /* 2 is not a filter, nor are 4, 5 and 7 */
enum { QOIMI_FILTER_NEAREST = 9 };   /* 8 is not a filter */
enum { QOIMI_FILTER_MODE = 11 };   /* 10 is not a filter */
typedef struct {                 /* 48 bytes, offsets 0/4/8/24/40 */
    unsigned int dtype;          /* QOIMI_TENSOR_* */
    unsigned int layout;         /* QOIMI_TENSOR_HWC / _CHW / _HW / _HW_ID24 */
    float scale[4];              /* per channel r, g, b, a */
    float bias[4];
    unsigned int reserved[2];    /* 0 */
} qoimi_tensor_format;
int qoimi_decode_tensors(qoimi_ctx *ctx, const void *d_streams, const size_t *stream_offsets /* host */, const int *sizes /* host */,
                         const qoi_desc *descs /* host */, int n_images, int channels /* 0, 3, 4 */,
                         const qoimi_resize *items /* host */, int n_items, int filter, int mode, const qoimi_tensor_format *format /* host */,
                         void *d_out, const size_t *out_offsets /* host, n_items */, size_t staging_bytes, void *stream);
int qoimi_decode_warped_tensors(qoimi_ctx *ctx, const void *d_streams, const size_t *stream_offsets /* host */, const int *sizes /* host */,
                                const qoi_desc *descs /* host */, int n_images, int channels /* 0, 3, 4 */,
                                const qoimi_warp *items /* host */, int n_items, int mode, const qoimi_tensor_format *format /* host */,
                                void *d_out, const size_t *out_offsets /* host, n_items */, size_t staging_bytes, void *stream);

/* out_width * out_height * channels * element size (QOIMI_TENSOR_HW, QOIMI_TENSOR_HW_ID24: out_width * out_height * element size) - the bytes of the item's output -
 * or 0 if filter is unknown, the format is one the calls reject, qoimi_resize_size / qoimi_bilinear_size (by filter) or qoimi_warp_size would
 * return 0, the item is beyond the limits of QOIMI_FILTER_BICUBIC, QOIMI_FILTER_LANCZOS, QOIMI_FILTER_NEAREST or QOIMI_FILTER_MODE with that filter, or the
 * product does not fit a size_t.  Pure
 * host arithmetic: no context, no GPU. */
size_t qoimi_tensor_size(const qoi_desc *desc, const qoimi_resize *item, int filter, int channels, const qoimi_tensor_format *format);
size_t qoimi_warp_tensor_size(const qoi_desc *desc, const qoimi_warp *item, int channels, const qoimi_tensor_format *format);

/* Of the context's last qoimi_decode_tensors or qoimi_decode_warped_tensors call, whichever came last: [0] sub-batches decoded, [1] launches
 * of its tensor kernel (it has no entry in qoimi_kernel_name), [2] bytes of the staging the call planned for (its largest sub-batch),
 * [3] images decoded (the referenced ones). */
void qoimi_tensor_stats(qoimi_ctx *ctx, long long out[4]);

/* What is in the pixels of rectangles of a pack's images, without the caller ever owning the decoded images: a tile server learns which tiles
 * of a scan are blank (a constant tile need not be stored) and which are fully opaque (they can be re-encoded with 3 channels), a training
 * loader gets the per-channel sums its normalisation needs and can drop empty or single-colour samples.  The referenced streams are decoded as
 * for qoimi_decode_crops - into the staging arena, sub-batch by sub-batch, down to the last row any region needs - and reduced there.
 * The result (normative; qoi_amd/pixelstats.py: stats states it in Python): decode stream regions[j].image exactly as qoimi_decode_images does
 * (same leniency, bit-exact for EVERY input stream) to 4 channels, which gives D of h rows of w pixels; the call has no channels argument, images
 * of both channel counts mix freely, and a 3-channel stream has alpha 255 everywhere (its regions are OPAQUE, sum[3] = 255 * pixels).  Region j is
 * D[y .. y + height) x [x .. x + width); stats_out[j] holds, over its pixels: their number, per channel r, g, b, a the sum, the sum of squares,
 * the minimum and the maximum, the numbers of pixels with a == 255, with a == 0 and with r == g == b, `first`, and the flags, which are a
 * function of the other fields.  The two FLIP bits of qoimi_crop are accepted and change nothing but `first`: it is pixel (0, 0) of the
 * FLIPPED rectangle, the first pixel qoimi_decode_crops would write.  All arithmetic is integer: the result is a function of the inputs alone.
 *   stream_offsets, sizes, descs  HOST arrays as for qoimi_decode_images.  An image that no region names is NOT decoded and its sizes[i] and
 *                  descs[i] are not even checked
 *   regions        HOST qoimi_crop[n_regions], in any order of image; several may name the same image, overlap or coincide: each has its own
 *                  result
 *   stats_out      HOST qoimi_pixel_stat[n_regions]
 *   d_hist         NULL, or DEVICE unsigned[n_regions][4][256]: d_hist[j][c][v] is the number of pixels of region j whose channel c is v (below
 *                  400 000 000).  Zeroed by the call; it stays on the device - 4 KiB per region are the caller's to copy or not.  With NULL
 *                  nothing of it is computed
 *   staging_bytes  as for qoimi_decode_crops: the arena qoimi_verify_images and the gather calls use, counted in qoimi_workspace_bytes [1],
 *                  allocated as the largest sub-batch of the call's plan plus a page; 4 bytes per pixel; 0: 1 GiB.  The plan is that of
 *                  qoimi_decode_crops over the regions (normative; qoi_amd/pixelstats.py: plan, which is qoi_amd/crops.py: plan)
 * Every sub-batch is one qoimi_decode_images call as it is, at 4 output channels and with each descriptor's height replaced by rows_i, then one
 * launch of the reduction kernel over all regions of the sub-batch's images on `stream`.
 * SYNCHRONOUS: returns when stats_out is filled and d_hist written.  The code of a decode sub-call that failed ends the call.  QOIMI_E_ARG for a
 * NULL ctx, d_streams, stream_offsets, sizes, descs, regions or stats_out, n_images <= 0, n_regions <= 0, regions[j].image >= n_images, a zero
 * width or height, a rectangle that leaves its image, a flag bit other than the two, a referenced stream shorter than 22 bytes, a rejected
 * referenced descriptor, a sub-batch of the plan with 2^31 - 1 or more tiles of 1024 pixels of a region: reported before anything is launched,
 * stats_out is untouched.  The sub-batches count as decode calls of the context, as those of qoimi_verify_images do.  One call at a time per
 * context, as everywhere. */
enum { QOIMI_PS_CONSTANT = 1,      /* every pixel of the rectangle equals `first` (all four bytes): min[c] == max[c] for c = 0..3 */
       QOIMI_PS_OPAQUE = 2,        /* opaque_pixels == pixels */
       QOIMI_PS_TRANSPARENT = 4,   /* transparent_pixels == pixels */
       QOIMI_PS_GREY = 8 };        /* grey_pixels == pixels (r == g == b everywhere) */
typedef struct {                          /* 128 bytes, offsets 0/8/40/72/76/80/84/88/96/104 */
    unsigned long long pixels;            /* width * height of the rectangle */
    unsigned long long sum[4];            /* per channel r, g, b, a */
    unsigned long long sum_sq[4];         /* per channel, sum of squares (<= 255^2 * 4e8 < 2^45) */
    unsigned char min[4], max[4];
    unsigned int first;                   /* pixel (0, 0) of the rectangle, r | g<<8 | b<<16 | a<<24 */
    unsigned int flags;                   /* QOIMI_PS_*: a function of the other fields, as stated above */
    unsigned long long opaque_pixels;     /* a == 255 */
    unsigned long long transparent_pixels;/* a == 0 */
    unsigned long long grey_pixels;       /* r == g && g == b */
    unsigned int reserved[4];             /* 0 */
} qoimi_pixel_stat;
int qoimi_pixel_stats(qoimi_ctx *ctx, const void *d_streams, const size_t *stream_offsets /* host */, const int *sizes /* host */,
                      const qoi_desc *descs /* host */, int n_images,
                      const qoimi_crop *regions /* host */, int n_regions,
                      qoimi_pixel_stat *stats_out /* host, n_regions */,
                      unsigned *d_hist /* DEVICE unsigned[n_regions][4][256], may be NULL */,
                      size_t staging_bytes, void *stream);

/* Of the context's last qoimi_pixel_stats call: [0] sub-batches decoded, [1] launches of the reduction kernel (it has no entry in
 * qoimi_kernel_name), [2] bytes of the staging the call planned for (its largest sub-batch), [3] images decoded (the referenced ones). */
void qoimi_pixel_stats_counters(qoimi_ctx *ctx, long long out[4]);

/* A row seek index: a band of an image without the rows above it.  The gather calls above stop at the last row a rectangle needs but start
 * at row 0 (every pixel depends on the one before): a 256-row band at the top of a 16384 x 16384 scan stages 16 MiB, the same band at the bottom
 * the whole image.  The decoder's state at a row boundary is small - the previous pixel, the 64-entry colour table, a byte position, what is left
 * of a run - so it can be kept (a SEEK POINT, 272 bytes) and written down as QOI chunks: a BAND STREAM is a header, at most 64 QOI_OP_RGBA chunks
 * that load the table and the previous pixel, QOI_OP_RUN chunks that pad to whole rows, and the original stream's bytes from the point on.  It is
 * an ordinary QOI stream; decoded by any decode call as it is, its rows from pad_rows on are the band's rows of the full decode, bit-exact for
 * EVERY input stream (cut streams, wrong end markers, hostile bodies: the leniency of qoi_decode carries over).
 * All of it (normative; qoi_amd/seekindex.py states it in Python).  For an image of w x h, a stream of `size` bytes, D its decode at 4 channels as
 * qoimi_decode_images gives it and an interval of K rows, K * w >= 128, the seek points are at the rows K, 2K, ... < h: ceil(h / K) - 1 of them,
 * possibly none.  Point k (from 0) sits at pixel P = (k + 1) * K * w and holds
 *   byte_off, skip  the walk of qoimi_inspect_streams: p = 14, end = size - 8, px = 0; while p < end: n = pixels of the chunk at p; px + n > P:
 *                   stop; else px += n, p += the chunk's length.  Stopped inside the body: byte_off = p, skip = P - px (0..61, non-zero only inside
 *                   a QOI_OP_RUN).  The walk ran out: byte_off = size - 8, skip = 0
 *   prev            pixel P - 1 of D as r | g << 8 | b << 16 | a << 24
 *   table[s]        the last pixel of D in front of P whose hash (3r + 5g + 7b + 11a) % 64 is s, else 0
 * The band stream of the band (first_row, rows) - first_row 0 or a seek row, first_row + rows <= h; e the point at first_row, e2 the first point
 * at a row >= first_row + rows, if there is one - is, concatenated: the header qoif, w, pad_rows + rows, the original channels and colorspace; for s
 * ascending every table[s] that is neither 0 nor prev as FF r g b a, then prev the same way (n <= 64 chunks); with pad_rows = max(1, ceil((n + skip)
 * / w)) and R = pad_rows * w - skip - n: R / 62 bytes 0xFD and, if R % 62 != 0, one byte 0xC0 | (R % 62 - 1); the original bytes [byte_off,
 * min(byte_off(e2) + 13, size)), up to size without e2.  first_row == 0: no loads, pad_rows = 0, the original bytes from 14 on.  pad_rows <= K always.
 * Costs, stated plainly: building an index from the streams alone (qoimi_build_seek_index) is one qoimi_inspect_streams plus one full decode of
 * every image that has a point; whoever still holds the pixels the pack was encoded from builds it without a decode
 * (qoimi_seek_index_from_pixels); an indexed call copies each band's stream bytes once.  Build it once per pack and keep 272 bytes per point
 * beside the pack's offsets. */
typedef struct { unsigned byte_off, skip, prev, reserved; unsigned table[64]; } qoimi_seek_point;   /* 272 bytes; reserved: 0 */
typedef struct { unsigned image, first_row, rows, reserved; } qoimi_band;                            /* 16 bytes; reserved is not looked at */
typedef struct { unsigned long long size; qoi_desc desc; unsigned pad_rows; } qoimi_band_info;       /* 24 bytes, offsets 0/8/20 */

/* ceil(height / interval_rows) - 1, the seek points of an image, or -1 if desc is rejected, interval_rows == 0 or interval_rows * width < 128.
 * Pure host arithmetic: no context, no GPU. */
int qoimi_seek_points(const qoi_desc *desc, unsigned interval_rows);

/* The seek points of every image of a pack.
 *   stream_offsets, sizes, descs  HOST arrays as for qoimi_decode_images
 *   interval_rows  HOST unsigned[n_images]: image i's K
 *   points_out     HOST qoimi_seek_point[sum of qoimi_seek_points(&descs[i], interval_rows[i])], the images' points back to back in image order
 *   staging_bytes  as for qoimi_decode_thumbnails: the arena of the gather calls, 4 bytes per pixel, slots of width * height * 4 rounded up to 256
 *                  bytes over the images that HAVE a point, in order, sub-batches cut by qoi_amd/packplan.py: plan; 0: 1 GiB
 * byte_off and skip come from the passes of qoimi_inspect_streams as they are, a scan of the pixels of their 16 KiB blocks and one wavefront per
 * point that walks one block (no stream is walked serially); prev and table from one qoimi_decode_images call per sub-batch as it is, at 4 output
 * channels, and two small kernels over the staged pixels.  Workspace beside the staging (counted in qoimi_workspace_bytes [1]): that of
 * qoimi_inspect_streams plus 8 bytes per 16 KiB block and 552 per point.  One wavefront per image walks that image's points in order (the
 * table is carried from point to point): the time of that step grows with the points of the image that has most, a few thousand are nothing, an
 * interval of one row on an image of millions of rows is millions of dependent steps - choose intervals of tens to hundreds of rows.
 * SYNCHRONOUS.  QOIMI_E_ARG for a NULL ctx, d_streams, stream_offsets, sizes, descs, interval_rows or points_out, n_images <= 0, sizes[i] < 22, a
 * rejected descriptor, interval_rows[i] * width < 128, 2^25 seek points or more, more than 2^31 blocks of stream bytes, 2^31 - 1 or more tiles of
 * 1024 pixels in a sub-batch:
 * reported before anything is launched, points_out is untouched.  The sub-batches count as decode calls of the context, as those of
 * qoimi_verify_images do.  One call at a time per context, as everywhere. */
int qoimi_build_seek_index(qoimi_ctx *ctx, const void *d_streams, const size_t *stream_offsets /* host */, const int *sizes /* host */,
                           const qoi_desc *descs /* host */, int n_images, const unsigned *interval_rows /* host, n_images */,
                           qoimi_seek_point *points_out /* host */, size_t staging_bytes, void *stream);

/* The seek points of every image of a pack whose PIXELS the caller holds on the device - it has just encoded the pack from them
 * (qoimi_encode_images_packed: packed_off_out / stream_len_out are this call's stream_offsets / sizes) - without decoding anything.
 *   d_pixels, pixel_offsets  as for qoimi_encode_images: image i is width * height * descs[i].channels bytes, tightly packed, at d_pixels +
 *                  pixel_offsets[i] - ANY byte offset; 3- and 4-channel images mix in one call.  Read only
 *   stream_offsets, sizes, descs, interval_rows, points_out  as for qoimi_build_seek_index
 * The result (normative; qoi_amd/seekindex.py: points_from_pixels): the points qoi_amd/seekindex.py: points gives with D the caller's pixels at 4
 * channels, alpha 255 where descs[i].channels == 3.  byte_off and skip are the walk of the STREAM, exactly as for qoimi_build_seek_index; prev
 * and table are taken from the PIXELS.  Whenever stream i decodes to those pixels - every stream this library or the reference encoder wrote
 * from them - the result is that of qoimi_build_seek_index, byte for byte.
 * An image's pixels are the caller's data.  CHECKED is what keeps every access inside the arguments: byte_off and skip always come from the
 * stream itself, so byte_off lies inside [14, size - 8] and skip is at most 61 whatever the pixels hold, and of the pixels nothing is read but
 * the aligned 4-byte words that hold a byte of an image.  TRUSTED and, where wrong, giving an index whose bands decode to wrong pixels and
 * nothing worse: that stream i decodes to the pixels at pixel_offsets[i] (qoimi_verify_images checks exactly that).
 * No qoimi_decode_images sub-call is made and the staging arena is not used: byte_off and skip from the passes of qoimi_inspect_streams and one
 * wavefront per point, as for qoimi_build_seek_index; prev and table from two kernels over the caller's pixels, ONE launch each for all images of
 * the call (there are no sub-batches; qoimi_seek_stats [0] is set to 0).  Workspace (counted in qoimi_workspace_bytes [1]): that of
 * qoimi_inspect_streams plus 8 bytes per 16 KiB block, 552 per point and 32 per image that has a point.  The remark on intervals of one row
 * there holds here too.
 * SYNCHRONOUS: one wait, at the end.  QOIMI_E_ARG for a NULL ctx, d_pixels, pixel_offsets, d_streams, stream_offsets, sizes, descs, interval_rows
 * or points_out, n_images <= 0, sizes[i] < 22, a rejected descriptor, interval_rows[i] * width < 128, an image whose last byte's address does not
 * fit in a pointer, 2^25 seek points or more, more than 2^31 blocks of stream bytes, 2^31 - 1 or more tiles of 1024 pixels in the call:
 * reported before anything is launched, points_out is untouched.  One call at a time per context, as everywhere. */
int qoimi_seek_index_from_pixels(qoimi_ctx *ctx, const void *d_pixels, const size_t *pixel_offsets /* host */,
                                 const void *d_streams, const size_t *stream_offsets /* host */, const int *sizes /* host */,
                                 const qoi_desc *descs /* host */, int n_images, const unsigned *interval_rows /* host, n_images */,
                                 qoimi_seek_point *points_out /* host */, void *stream);

/* What the band stream of `band` will be: its size, its descriptor (width, pad_rows + rows, the image's channels and colorspace) and pad_rows -
 * from the points alone, without the stream's bytes.  points: this image's (may be NULL where the band uses none: an image without points);
 * band->image is not looked at.  0 on success; QOIMI_E_ARG for a NULL desc, band or out, a rejected descriptor, size < 22, interval_rows * width <
 * 128, a first_row that is neither 0 nor a seek row, rows == 0, first_row + rows > height, a band stream of 2^31 - 1 bytes or more, and a point
 * the band uses that cannot be one.  An index is the caller's data; of the points a band uses (e, e2; the others are not read) exactly this is
 * CHECKED, and it is what keeps every read inside the stream and every write inside the band stream: byte_off inside [14, size - 8], skip <= 61,
 * byte_off(e2) + 13 >= byte_off(e), and n <= 64 loads for e (a point of a stream holds prev in prev's own slot; 64 table words that are all
 * non-zero and differ from prev would be 65 loads).  Everything else is TRUSTED and, where wrong, gives wrong pixels and nothing worse: that
 * byte_off is a chunk's first byte of THIS stream, that skip, prev and the table words are the decoder's state there, that reserved is 0.
 * Pure host arithmetic: no context, no GPU. */
int qoimi_band_plan(const qoi_desc *desc, int size, unsigned interval_rows, const qoimi_seek_point *points /* this image's */,
                    const qoimi_band *band, qoimi_band_info *out);

/* Band streams, written on the device: band stream j - infos_out[j].size bytes, what qoimi_band_plan says - at d_out + out_offsets[j].
 *   stream_offsets, sizes, descs, interval_rows  HOST arrays over the n_images images, as for qoimi_build_seek_index; an image that no band names
 *                  is not checked and its points are not read
 *   points         HOST, the index; point_firsts HOST size_t[n_images]: image i's points begin at points[point_firsts[i]]
 *   bands          HOST qoimi_band[n_bands], in any order; several may name the same image
 *   out_offsets    HOST size_t[n_bands]: ANY byte offsets in any order; not one byte beside a band stream is written (two may share an aligned
 *                  word: no word is ever read and written back); the ranges must not overlap each other or a stream a band names
 *   infos_out      HOST qoimi_band_info[n_bands], may be NULL
 * The caller's index is input and is checked as qoimi_band_plan checks it (byte_off, skip, the order of a band's two points, the number of
 * loads - see there for what is checked and what is trusted): whatever it holds, nothing outside [stream_offsets[i], + sizes[i]) is read - but
 * for the aligned 4-byte words that hold a first or last byte - and nothing beside the band streams is written.  A band stream made from another stream's index is still a stream
 * every decode call accepts; its pixels are then not the band's.
 * SYNCHRONOUS.  QOIMI_E_ARG for a NULL ctx, d_streams, stream_offsets, sizes, descs, interval_rows, points, point_firsts, bands, d_out or
 * out_offsets, n_images <= 0, n_bands <= 0, more than 12 782 640 bands, bands[j].image >= n_images, whatever qoimi_band_plan rejects, overlapping ranges, 2^31 - 1 or more
 * tiles of 256 aligned 16-byte words of output: reported before anything is launched, the caller's buffers are untouched. */
int qoimi_make_band_streams(qoimi_ctx *ctx, const void *d_streams, const size_t *stream_offsets /* host */, const int *sizes /* host */,
                            const qoi_desc *descs /* host */, int n_images, const unsigned *interval_rows /* host */,
                            const qoimi_seek_point *points /* host */, const size_t *point_firsts /* host, n_images */,
                            const qoimi_band *bands /* host */, int n_bands, void *d_out, const size_t *out_offsets /* host, n_bands */,
                            qoimi_band_info *infos_out /* host, may be NULL */, void *stream);

/* qoimi_decode_crops, byte for byte, decoding each referenced image only from the last seek row at or above its topmost crop.
 * (normative; qoi_amd/seekindex.py: bands_for_crops): per referenced image i, K = interval_rows[i], first_row = (the smallest y of its crops) / K
 * * K, rows = (the largest y + height) - first_row.  The band streams of these bands are assembled into an arena of the context (counted in
 * qoimi_workspace_bytes [1]; planned as the sum of the band streams' sizes, each rounded up to 16 - qoimi_seek_stats [2] - and allocated as
 * that plus a page, no slack), then qoimi_decode_crops runs as it is over
 * them: the band streams are the streams, their descriptors the descriptors, the referenced images numbered in ascending order, every crop's y
 * replaced by y - first_row + pad_rows.  The sub-batch plan and the counters of qoimi_crop_stats are those of that inner call: [2] shows the
 * saving.  Arguments and rejections of qoimi_decode_crops, and for the referenced images those of qoimi_make_band_streams (an image that no crop
 * names is not checked and its points are not read); QOIMI_E_ARG also for a NULL interval_rows, points or point_firsts and for more than
 * 12 782 640 referenced images.  SYNCHRONOUS. */
int qoimi_decode_crops_indexed(qoimi_ctx *ctx, const void *d_streams, const size_t *stream_offsets /* host */, const int *sizes /* host */,
                               const qoi_desc *descs /* host */, int n_images, int channels /* 0, 3, 4 */,
                               const qoimi_crop *crops /* host */, int n_crops,
                               void *d_out, const size_t *out_offsets /* host, n_crops */, size_t staging_bytes, void *stream,
                               const unsigned *interval_rows /* host, n_images */, const qoimi_seek_point *points /* host */,
                               const size_t *point_firsts /* host, n_images */);

/* qoimi_decode_resized and qoimi_pixel_stats, byte for byte - `first` and the flags of the statistics included - decoding each referenced image
 * only from the last seek row at or above its topmost item: a tile of fixed size at any zoom, or "which tiles of a scan are blank", without the
 * rows above the tiles.  Exactly as qoimi_decode_crops_indexed (normative; qoi_amd/seekindex.py: bands_for_crops over the items' SOURCE
 * rectangles x, y, width, height): the bands are assembled into the context's band arena, then the plain call runs as it is over them, `image`
 * renumbered and every y replaced by y - first_row + pad_rows.  The sub-batch plan and the counters of qoimi_resize_stats /
 * qoimi_pixel_stats_counters are those of that inner call; qoimi_seek_stats [1..3] are set as qoimi_decode_crops_indexed sets them.  Arguments
 * and rejections of the plain call, and for the referenced images those of qoimi_make_band_streams (an image that no item names is not checked
 * and its points are not read; what of an index is checked and what is trusted: qoimi_band_plan); QOIMI_E_ARG also for a NULL interval_rows,
 * points or point_firsts and for more than 12 782 640 referenced images.  SYNCHRONOUS. */
int qoimi_decode_resized_indexed(qoimi_ctx *ctx, const void *d_streams, const size_t *stream_offsets /* host */, const int *sizes /* host */,
                                 const qoi_desc *descs /* host */, int n_images, int channels /* 0, 3, 4 */,
                                 const qoimi_resize *items /* host */, int n_items, int mode,
                                 void *d_out, const size_t *out_offsets /* host, n_items */, size_t staging_bytes, void *stream,
                                 const unsigned *interval_rows /* host, n_images */, const qoimi_seek_point *points /* host */,
                                 const size_t *point_firsts /* host, n_images */);
/* qoimi_decode_bilinear byte for byte, exactly as qoimi_decode_resized_indexed: band assembly over the items' SOURCE rectangles, then the plain
 * call as it is with `image` renumbered and every y replaced by y - first_row + pad_rows.  The counters of qoimi_bilinear_stats are those of the
 * inner call; qoimi_seek_stats [1..3] are set as qoimi_decode_crops_indexed sets them.  SYNCHRONOUS. */
int qoimi_decode_bilinear_indexed(qoimi_ctx *ctx, const void *d_streams, const size_t *stream_offsets /* host */, const int *sizes /* host */,
                                  const qoi_desc *descs /* host */, int n_images, int channels /* 0, 3, 4 */,
                                  const qoimi_resize *items /* host */, int n_items, int mode,
                                  void *d_out, const size_t *out_offsets /* host, n_items */, size_t staging_bytes, void *stream,
                                  const unsigned *interval_rows /* host, n_images */, const qoimi_seek_point *points /* host */,
                                  const size_t *point_firsts /* host, n_images */);
/* qoimi_decode_warped byte for byte, exactly as qoimi_decode_resized_indexed: band assembly over the items' SOURCE rectangles, then the plain
 * call as it is with `image` renumbered and every y replaced by y - first_row + pad_rows (the map is relative to the rectangle and stays).  The
 * counters of qoimi_warp_stats are those of the inner call; qoimi_seek_stats [1..3] are set as qoimi_decode_crops_indexed sets them.
 * SYNCHRONOUS. */
int qoimi_decode_warped_indexed(qoimi_ctx *ctx, const void *d_streams, const size_t *stream_offsets /* host */, const int *sizes /* host */,
                                const qoi_desc *descs /* host */, int n_images, int channels /* 0, 3, 4 */,
                                const qoimi_warp *items /* host */, int n_items, int mode,
                                void *d_out, const size_t *out_offsets /* host, n_items */, size_t staging_bytes, void *stream,
                                const unsigned *interval_rows /* host, n_images */, const qoimi_seek_point *points /* host */,
                                const size_t *point_firsts /* host, n_images */);
int qoimi_pixel_stats_indexed(qoimi_ctx *ctx, const void *d_streams, const size_t *stream_offsets /* host */, const int *sizes /* host */,
                              const qoi_desc *descs /* host */, int n_images,
                              const qoimi_crop *regions /* host */, int n_regions,
                              qoimi_pixel_stat *stats_out /* host, n_regions */,
                              unsigned *d_hist /* DEVICE unsigned[n_regions][4][256], may be NULL */,
                              size_t staging_bytes, void *stream,
                              const unsigned *interval_rows /* host, n_images */, const qoimi_seek_point *points /* host */,
                              const size_t *point_firsts /* host, n_images */);

/* [0] sub-batches decoded by the context's last qoimi_build_seek_index (qoimi_seek_index_from_pixels: 0), [1] band streams assembled by its
 * last qoimi_make_band_streams or indexed call (qoimi_decode_crops_indexed, qoimi_decode_resized_indexed, qoimi_decode_bilinear_indexed, qoimi_pixel_stats_indexed), [2] bytes of the band arena that call planned for (qoimi_make_band_streams: 0), [3] stream bytes it copied (the
 * tails).  The kernels have no entry in qoimi_kernel_name. */
void qoimi_seek_stats(qoimi_ctx *ctx, long long out[4]);

/* Fill device memory with synthetic RGBA frames frame_id = first_frame .. first_frame+n-1
 * (benchmark/test utility; same function of (kind, seed, frame, pixel) as synth.py). */
int qoimi_synth_frames(qoimi_ctx *ctx, int kind, unsigned seed, unsigned first_frame,
                       int n_frames, unsigned width, unsigned height,
                       void *d_pixels, size_t pixel_stride, void *stream);

/* 64-bit content hash of n_streams streams in device memory (stream i: d_stream_len[i] bytes at d_streams + i*stream_stride),
 * written to the device array d_hash[n_streams]; asynchronous on `stream`.  Benchmark / test utility: whole batches are compared
 * with hashes of the REFERENCE encoder's streams without copying the streams out (bench.py, qoi_amd/synth.py: stream_hash64 states
 * the function: sum over the 8-byte little-endian words w_j, last one zero-padded, of splitmix64(w_j + (j+1) * 0x9E3779B97F4A7C15)). */
int qoimi_hash_streams(qoimi_ctx *ctx, const void *d_streams, size_t stream_stride, const int *d_stream_len, int n_streams,
                       unsigned long long *d_hash, void *stream);

/* Device memory the context's growable arenas hold at the moment (bytes): [0] encode workspace (and the staging arena of
 * qoimi_encode_packed and qoimi_encode_tiles, which holds the gathered tiles, their strided streams and the tile table), [1] decode workspace
 * (and the tables of qoimi_inspect_streams, the tables of qoimi_compare_images, the tables and the staging arena of qoimi_verify_images,
 * qoimi_decode_thumbnails, qoimi_decode_crops, qoimi_decode_resized, qoimi_decode_bilinear, qoimi_pixel_stats and qoimi_build_seek_index, which share them, the tables of
 * qoimi_build_seek_index and qoimi_seek_index_from_pixels and the band arena of the indexed calls),
 * [2] staging buffers of the host-pointer entry points (qoi_encode / qoi_decode of the calling thread's context). */
void qoimi_workspace_bytes(qoimi_ctx *ctx, size_t out[3]);

/* Caps the chunk-record arena of this context's decode calls (bytes; at least 1 MiB): a call whose streams need more - four bytes
 * per stream byte, the worst case - is decoded as consecutive sub-batches of whole images through the same arena, and `release`
 * != 0 gives the arena grown so far back to the device.  Default: a sixth of the device's memory, 48 GiB at most (1024 4K
 * photographs in one piece: 45 GB of workspace); 24 GiB decodes them as two sub-batches in 27 GB at +1 % of the time
 * (DESIGN.md section 4).  The pixels are the same either way.  Returns QOIMI_OK or QOIMI_E_ARG. */
int qoimi_set_decode_record_cap(qoimi_ctx *ctx, size_t bytes, int release);

/* Counters of the last decode on this context: [0] speculation rounds, [1] segments
 * re-decoded after a failed check, [2] total segments, [3] segments whose entry position
 * needed the full five-phase parse (look-back synchronisation did not settle). */
void qoimi_decode_stats(qoimi_ctx *ctx, long long out[4]);

/* Per-kernel timing with HIP events recorded on the launch stream (what bench.py's roofline
 * figure is computed from).  qoimi_set_profiling(ctx,1) enables it and resets the
 * accumulators; qoimi_get_profile synchronises `stream` and returns, per kernel index,
 * accumulated milliseconds and launch counts (arrays of `cap` entries; return value =
 * number of kernels); qoimi_kernel_name(i) names index i. */
int qoimi_set_profiling(qoimi_ctx *ctx, int on);
int qoimi_get_profile(qoimi_ctx *ctx, void *stream, double *ms, long long *calls, int cap);
const char *qoimi_kernel_name(int index);

/* Library/version string, e.g. "qoi_mi355x 0.1 gfx950". */
const char *qoimi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* QOI_MI355X_H */
