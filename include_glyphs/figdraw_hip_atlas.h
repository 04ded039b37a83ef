/* figdraw_hip_atlas.h -- atlas compaction for libfigdraw_hip.so: repack or resize the image atlas with every live entry KEPT.  Same
 * conventions as figdraw_hip.h (plain C, every call returns 0 or a negative FdhStatus, fdh_last_error() says why).  The header lives in
 * include_glyphs/ beside the glyph headers and reaches figdraw_hip.h by its relative path: -I include_glyphs is all a caller adds.
 *
 * Why.  The atlas forgets in two ways.  A put that does not fit doubles the atlas and drops every entry (figdraw_hip.h at fdh_put_image:
 * the reference's rule), and fdh_remove_image erases a directory entry while the packer's skyline never comes down.  The texels of this
 * library's atlas were made on the GPU and live there: making 376 glyph variants and 106 fields again because one icon did not fit is the
 * whole glyph pipeline, moving them is a few launches from device memory to device memory.
 *
 * This comment is the specification.
 *
 * fdh_compact_atlas(ctx, size, stats).  `size` 0: the current size; else 1 .. 16384, rounded up to a power of two, smaller or larger than
 * the current size; anything else is FDH_ERR_INVALID.  The live entries are placed into an empty atlas of that size by the packer every
 * put uses (same margin, same skyline search), in COMPACTION ORDER: height descending, then width descending, then key ascending as a
 * signed 64-bit integer.
 * - If they do not all fit: FDH_ERR_ATLAS_FULL, and nothing has changed -- size, levels, directory, skyline, rectangles, epoch.
 * - If they fit: the new levels are allocated and cleared first (a failed allocation leaves the old atlas whole), the texels are moved,
 *   the old levels are freed, the directory holds the new positions with the ink boxes and everything else of an entry kept, and the
 *   epoch moves: cached records of retained scenes are rebuilt.  The out_rect of earlier puts is stale: fdh_image_rect.
 * The call waits for the context's submit thread and its stream like every put: a frame in flight is finished from the old atlas.  On a
 * record-only context the directory and the packer do the same and no device is touched.
 *
 * The contract.  After a successful call every level of the atlas is byte for byte what a fresh context of that size holds after the same
 * puts (the same put call with the same arguments) of the live entries, made in compaction order; so are the directory, the rectangles,
 * fdh_atlas_packed_area and the ink boxes.  Texels of removed entries are gone: the new levels start cleared.  A level texel that the
 * rectangles of two entries share belongs to the later entry in compaction order, as single puts leave it.
 *
 * How the texels move, and why it is not a plain copy of every level.  Level 0 rectangles never meet (the packer keeps 8 texels between
 * images), deeper ones do: level l stores ceil(w / 2^l) texels at x >> l, and from level 4 on the last column or row of one image's
 * rectangle is the first of its neighbour's.  Such a texel holds what the LATER put wrote; the earlier image's own value is nowhere in the
 * old atlas -- it may even belong to an entry that was removed since.  A copy would carry a neighbour's texel into a place where the
 * fresh context holds the image's own.  So:
 * - level 0 of every entry is copied (k_atlas_move: one launch for all entries);
 * - levels 1 .. of an entry whose put built the level chain (fdh_put_image, fdh_update_image, fdh_put_glyph_image, every outline, field
 *   and batch put) are built again from its level 0 by the chain's own kernels, for all entries at once: one blit and one minify per
 *   level, the launches of a batch put.  The chain is a function of the image alone, so these are the bytes the put made;
 * - levels 1 .. of an entry of fdh_put_image_mips or fdh_put_flippy, whose sizes and texels are the caller's and need not be a chain, come
 *   from a copy of those levels that the atlas keeps in host memory from the put on (a third of the image), in one more launch of
 *   k_atlas_move.  A level is stored where a put into the new atlas stores it: while the atlas has that level and the rectangle at
 *   (x >> l, y >> l) stays inside it.  fdh_update_image of such an entry makes it a chain entry.
 * Shared texels go by owner bits worked out on the host from the destination rectangles, painted in compaction order.
 *
 * fdh_set_atlas_keep(ctx, on), off by default; when off nothing changes in any byte.  When on, a call whose image or images do not fit
 * the atlas as it stands -- where the placement would have grown it and dropped every entry -- first does this: take the smallest size
 * S' in {S, 2S, .. 16384} at which a trial packing fits (host only, on a scratch skyline: the live entries in compaction order, then the
 * image or images the call is about to place, in call order), run fdh_compact_atlas(S'), then make the call as ever.  S' = S happens when
 * removed entries left the room: the atlas grows only when live content needs it.  For a batch call "the images" are all glyphs of the
 * batch: the compaction happens once, before any glyph is placed, and moves only entries that have their texels; the batch then no longer
 * grows, and its own contract -- equality with single calls -- holds from that point unchanged.  A growing batch in keep mode is NOT
 * equal to growing single calls in keep mode: singles compact before each call that does not fit, the batch once for all its glyphs, and
 * the layouts legitimately differ.  If no size up to 16384 fits, the atlas is compacted to 16384 and the call proceeds: the placement
 * throws FDH_ERR_ATLAS_FULL where it always did, and a batch's earlier glyphs get their texels as today.  fdh_put_image_sdf_of keeps
 * copying its source to scratch first: the source may move.
 *
 * fdh_image_rect: where an entry is now.  fdh_atlas_usage: the reference's atlasUsage (figbackend.nim:304-333) -- used area against
 * packed area tells an application when a compaction pays.  fdh_debug_read_atlas_level: one whole level, for tests. */
#ifndef FIGDRAW_HIP_ATLAS_H
#define FIGDRAW_HIP_ATLAS_H
#include "../include/figdraw_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* what the last move did (fdh_compact_atlas fills it; on a record-only context the entries, the sizes, the areas and us_pack, the rest 0) */
typedef struct FdhAtlasMoveStats {
  int32_t entries;       /* live entries, all of them placed anew */
  int32_t rects_moved;   /* level rectangles written into the new atlas */
  int64_t texels;        /* their texels */
  int32_t tiles;         /* tiles (workgroups) of the k_atlas_move launches: 8 x 8 texels, 64 x 4 for rectangles at least 64 wide */
  int32_t launches;      /* kernel launches: k_atlas_move once, or twice when an fdh_put_image_mips / fdh_put_flippy entry has levels below 0, and two per atlas level for the chains */
  int32_t size_before, size_after;
  int64_t packed_before, packed_after;  /* fdh_atlas_packed_area */
  /* where the call's time went, host clock, microseconds: the compaction order and the trial packing; allocating and clearing the new
   * levels and freeing the old ones; building the tables; their upload, the launches and the wait for the stream */
  int32_t us_pack, us_alloc, us_tables, us_move;
} FdhAtlasMoveStats;

typedef struct FdhAtlasUsage {
  int32_t size;
  int32_t entries;
  int64_t used_area;     /* the sum of w x h of the live entries */
  int64_t packed_area;   /* fdh_atlas_packed_area: the area under the skyline */
  uint64_t epoch;        /* moves with every put, update, removal, reset and compaction */
  int64_t rebuilds;      /* times every entry was dropped: a growth without keep, fdh_reset_atlas */
  int64_t compactions;   /* successful fdh_compact_atlas runs, those of keep mode included */
} FdhAtlasUsage;

FDH_API int fdh_compact_atlas(FdhContext*, int size, FdhAtlasMoveStats* out_or_null);
FDH_API int fdh_set_atlas_keep(FdhContext*, int on);
FDH_API int fdh_get_atlas_keep(FdhContext*, int* out);
/* out_rect = x, y, w, h of the entry as it is placed now; an unknown key: FDH_ERR_INVALID */
FDH_API int fdh_image_rect(FdhContext*, int64_t key, int out_rect[4]);
FDH_API int fdh_atlas_usage(FdhContext*, FdhAtlasUsage* out);
/* level `level` of the atlas, (size >> level)^2 RGBA8 texels, rows packed; capacity_bytes below that, or a level the atlas does not
 * have: FDH_ERR_INVALID; a record-only context: FDH_ERR_NO_DEVICE */
FDH_API int fdh_debug_read_atlas_level(FdhContext*, int level, uint8_t* out, int64_t capacity_bytes);

#ifdef __cplusplus
}
#endif
#endif
