/*
 * lifeapi_hip.h -- C ABI of the MI355X (gfx950) batched LifeState::Step().
 *
 * The reference (scorbiclife/LifeAPI) is a header-only C++ library with no
 * FFI; its "operator API" is the inline member functions of LifeState.  Each
 * entry point below is the batched, device-resident replacement for one of
 * them, cited as file:line into the reference snapshot:
 *
 *   lifeapi_step_batch[_dev]     LifeState::Step()          LifeAPI.hpp:1196-1216
 *                                LifeState::Step(unsigned)  LifeAPI.hpp:877-881
 *                                LifeState::Stepped(unsigned) LifeAPI.hpp:882-886
 *   lifeapi_pop_batch_dev        LifeState::GetPop()        LifeAPI.hpp:290-298
 *   lifeapi_contains_batch_dev   LifeState::Contains(const LifeTarget&)
 *                                                           LifeTarget.hpp:44-51
 *   lifeapi_match_batch[_dev]    LifeState::Match(const LifeTarget&)
 *                                                           LifeTarget.hpp:53-55
 *                                LifeState::MatchLiveAndDead LifeAPI.hpp:432-435
 *                                LifeState::MatchLive, Match(const LifeState&)
 *                                                           LifeAPI.hpp:427-442
 *   lifeapi_convolve_batch[_dev] LifeState::Convolve        LifeAPI.hpp:1293-1370
 *                                (ZOI, BigZOI, NZOI are this with a fixed pattern)
 *   lifeapi_interaction_offsets_batch[_dev]
 *                                LifeState::InteractionOffsets LifeAPI.hpp:1066-1095
 *   lifeapi_transform_batch[_dev] LifeState::Transform, Transformed
 *                                                           Symmetry.hpp:105-173
 *                                LifeState::Move, Moved, FlipX, FlipY,
 *                                Transpose, Mirrored        LifeAPI.hpp:682-806
 *   lifeapi_symmetricize_batch[_dev] Symmetricize, PerpComponent
 *                                                           Symmetry.hpp:540-654
 *   lifeapi_transform_offsets_batch[_dev], lifeapi_symmetricize_offsets_batch[_dev]
 *                                the two above with an offset per universe
 *   lifeapi_convolve_pair_batch[_dev] a.Convolve(b.Transformed(t)), both per universe
 *   lifeapi_intersecting_offsets_batch[_dev]
 *                                IntersectingOffsets        Symmetry.hpp:729-772
 *   lifeapi_halve_batch[_dev]    LifeState::Halve, HalveX, HalveY
 *                                                           Symmetry.hpp:681-709
 *   lifeapi_skew_batch[_dev]     LifeState::Skew, InvSkew   Symmetry.hpp:711-727
 *   lifeapi_bounds_batch[_dev]   LifeState::XYBounds        LifeAPI.hpp:446-484
 *   lifeapi_symmetry_orbit_batch[_dev]
 *                                LifeState::SymmetryOrbit, SymmetryOrbitRepresentatives
 *                                                           Symmetry.hpp:798-830
 *   lifeapi_first_on_batch[_dev] LifeState::FirstOn, FirstCell LifeAPI.hpp:301-323, 358
 *   lifeapi_component_containing_batch[_dev]
 *                                LifeState::ComponentContaining
 *                                                           LifeAPI.hpp:655-665, 1184-1188
 *   lifeapi_components_batch[_dev] LifeState::Components    LifeAPI.hpp:667-676, 1189-1193
 *   lifeapi_weld_from_required_batch[_dev]
 *                                LifeWeld::FromRequired     LifeWeld.hpp:133-159
 *   lifeapi_weld_to_target_batch[_dev] LifeWeld::ToTarget   LifeWeld.hpp:188-191
 *   lifeapi_weld_to_stable_batch[_dev] LifeWeld::ToStable() LifeWeld.hpp:279-325
 *                                LifeWeld::ToStable(active, duration, mask)
 *                                                           LifeWeld.hpp:327-400
 *   lifeapi_weld_interaction_offsets_batch[_dev]
 *                                LifeWeld::InteractionOffsets(const LifeWeld &)
 *                                                           LifeWeld.hpp:206-245
 *   lifeapi_stable_strip_pass_batch[_dev]
 *                                LifeStable::*Strip passes  LifeStable.hpp:921-948, 995-1249
 *   lifeapi_stable_test_unknowns_batch[_dev]
 *                                LifeStable::TestUnknowns   LifeStable.hpp:1321-1338
 *                                (TestUnknown LifeStable.hpp:1251-1284, Join LifeStable.hpp:217-233)
 *   lifeapi_stable_propagate_and_test_batch[_dev]
 *                                LifeStable::PropagateAndTest LifeStable.hpp:163-184
 *   lifeapi_fill_random_dev      LifeState::RandomState()   LifeAPI.hpp:63-69
 *                                (seeded splitmix64; mode 1 = RandomState's
 *                                 [2^61, 2^62) column distribution)
 *   lifeapi_parse_rle_batch[_dev] LifeState::Parse          Parsing.hpp:143-198
 *   lifeapi_rle_*batch[_dev]     LifeState::RLE()           Parsing.hpp:8-63,200-204
 *   lifeapi_hash_batch_dev       (build-defined digest; stands in for
 *                                 LifeState::GetHash, LifeAPI.hpp:373, which
 *                                 needs the un-vendored xxHash)
 *
 * Data layout: a universe is the reference's LifeState, i.e. uint64_t[64]
 * (word x = column x, bit y = row y; LifeAPI.hpp:39-40,131), 512 bytes.  A
 * batch is a contiguous array of n universes = n*64 words.  Pointers must be
 * 8-byte aligned (LifeState is 64-byte aligned, so a LifeState[] always is).
 * in == out is allowed (in-place, like Step()); any other overlap is rejected.
 *
 * Conventions: every function returns 0 on success; a negative LIFEAPI_E_*
 * for a caller error; a positive hipError_t from the HIP runtime otherwise.
 * lifeapi_last_error() gives this thread's message for the last failure.
 * Nothing throws across this ABI.  The library owns only internal staging
 * buffers and streams (one per device, created lazily); the caller owns all
 * arguments.  *_dev functions take device pointers and enqueue on `stream`
 * (a hipStream_t; NULL = the null stream) without synchronising.  The host
 * functions are synchronous and thread-safe (one lock per device).
 */
#ifndef LIFEAPI_HIP_H
#define LIFEAPI_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LIFEAPI_ABI_VERSION 2

#define LIFEAPI_OK 0
#define LIFEAPI_E_INVALID (-1)   /* null/misaligned pointer, overlap, bad argument */
#define LIFEAPI_E_NODEVICE (-2)  /* no gfx950 device / bad device index */
#define LIFEAPI_E_NOKERNEL (-3)  /* code object for this GPU missing */

int lifeapi_abi_version(void);
const char *lifeapi_last_error(void);
int lifeapi_device_count(void);
/* which shipped kernel configuration lifeapi_step_batch[_dev] runs for this
 * many generations on a batch of n universes (the launch shape changes with
 * the batch size above 4M universes; a static string, for logs and benchmark
 * records); lifeapi_step_kernel_name(g) is the name for batches of at most 4M */
const char *lifeapi_step_kernel_name_n(uint32_t generations, size_t n);
const char *lifeapi_step_kernel_name(uint32_t generations);

/* ---- device-resident, stream-ordered (the hot path) -------------------- */

/* out[u] = in[u] stepped `generations` times (0 = copy), for u < n.  For
 * 1-2 generations and n >= 192K a call whose input is a batch an
 * earlier call wrote walks it in the opposite order to that call (a per-device
 * book of the last batches written; a cache-locality choice for back-to-back
 * calls on the batch just written); from 512K up to 2M and from 4M on each
 * XCD takes a contiguous eighth of the batch.  Results never depend on either, and
 * calls from several threads are safe.                                    */
int lifeapi_step_batch_dev(const uint64_t *d_in, uint64_t *d_out, size_t n,
                           uint32_t generations, void *stream);
/* d_pop[u] = population of universe u                                     */
int lifeapi_pop_batch_dev(const uint64_t *d_states, uint32_t *d_pop, size_t n, void *stream);
/* d_hash[u] = build-defined 64-bit hash of universe u     */
int lifeapi_hash_batch_dev(const uint64_t *d_states, uint64_t *d_hash, size_t n, void *stream);
/* d_out[u] = Contains(target) for target = (wanted, unwanted), both device
 * pointers to 64 words (LifeTarget.hpp:44-51).  Only the columns holding the
 * target's care cells (wanted | unwanted) are read from each universe.  With
 * unwanted = 0 this is Contains(pat), with wanted = 0 AreDisjoint(pat)
 * (LifeAPI.hpp:377-397); the (dx, dy) forms are these on the pattern moved by
 * (dx, dy) (LifeAPI.hpp:399-421).                                           */
int lifeapi_contains_batch_dev(const uint64_t *d_states, const uint64_t *d_wanted,
                               const uint64_t *d_unwanted, uint8_t *d_out, size_t n,
                               void *stream);
/* fused Step^gens + Contains: d_out[u] = first generation g in 1..gens at
 * which Stepped(g) contains the target, or 0 if none (all 0 for gens = 0);
 * d_final (may be NULL) receives Stepped(gens).  With d_final NULL (the
 * search filter) only the target's light cone is read and stepped: at 1-2
 * generations the columns within gens of its care columns, from 3 the
 * columns of a cone of at most 32 columns and the rows of a cone that fits
 * 32 rows; a target with neither is stepped whole.  Nothing is remembered
 * between calls: the target buffers may be rewritten between them.         */
int lifeapi_step_contains_batch_dev(const uint64_t *d_in, uint64_t *d_final,
                                    const uint64_t *d_wanted, const uint64_t *d_unwanted,
                                    uint32_t *d_first_gen, size_t n, uint32_t generations,
                                    void *stream);
/* d_out[u] = states[u].Match(LifeTarget{wanted, unwanted}) (LifeTarget.hpp:53-55,
 * LifeAPI.hpp:432-435): bit y of word x set iff the target moved by (x, y) is
 * contained.  d_count (may be NULL) receives the number of matches per universe;
 * d_out may be NULL when d_count is not (nothing but 4 bytes per universe is
 * written then); both NULL is an error.  An empty plane is vacuously
 * satisfied; d_out may be d_states.  Time is proportional to the target's
 * care cells (match_kernels.hpp).                                          */
int lifeapi_match_batch_dev(const uint64_t *d_states, const uint64_t *d_wanted,
                            const uint64_t *d_unwanted, uint64_t *d_out, uint32_t *d_count,
                            size_t n, void *stream);
/* d_out[u] = states[u].Convolve(pattern) (LifeAPI.hpp:1293-1370); one pattern
 * of 64 device words for the batch; d_out may be d_states                   */
int lifeapi_convolve_batch_dev(const uint64_t *d_states, const uint64_t *d_pattern,
                               uint64_t *d_out, size_t n, void *stream);
/* d_out[u] = states[u].InteractionOffsets(other) (LifeAPI.hpp:1066-1095)        */
int lifeapi_interaction_offsets_batch_dev(const uint64_t *d_states, const uint64_t *d_other,
                                          uint64_t *d_out, size_t n, void *stream);
/* d_out[u] = d_in[u].Transformed(transform).Moved(dx, dy)
 * (Symmetry.hpp:105-173, LifeAPI.hpp:682-735).
 * transform: the SymmetryTransform's value, 0..15 (Symmetry.hpp:7-26).
 * dx, dy: any int (Move wraps).
 * With transform 0 this is Moved; 1 FlipX; 3 FlipY; 13 / 14 Transpose(false / true).
 * Rotate180OddBoth (9) is Mirrored.  d_out may be d_in.                     */
int lifeapi_transform_batch_dev(const uint64_t *d_in, uint64_t *d_out, size_t n, uint32_t transform,
                                int dx, int dy, void *stream);
/* d_out[u] = Symmetricize(d_in[u], symmetry, {dx, dy}) (Symmetry.hpp:565-654).
 * symmetry: the StaticSymmetry's value (Symmetry.hpp:57-79): C1 0, D2AcrossX 1,
 * D2AcrossY 3, D2negdiagodd 5, D2diagodd 6, C2 7, C4 11, D4 13, D4diag 17.
 * LIFEAPI_E_INVALID for the symmetries the reference leaves undefined.
 * d_out may be d_in.                                                        */
int lifeapi_symmetricize_batch_dev(const uint64_t *d_in, uint64_t *d_out, size_t n, uint32_t symmetry,
                                   int dx, int dy, void *stream);
/* The two calls above with an offset per universe: d_offsets is n x {dx, dy}
 * int32 device words, any values (Move wraps; PerpComponent, Symmetry.hpp:540-563,
 * does not reduce mod 64), universe u taking d_offsets[2u], d_offsets[2u + 1].
 * d_out may be d_in; d_offsets overlapping d_out is LIFEAPI_E_INVALID; the
 * transforms and symmetries accepted are those of the calls above.          */
int lifeapi_transform_offsets_batch_dev(const uint64_t *d_in, uint64_t *d_out, size_t n,
                                        uint32_t transform, const int32_t *d_offsets, void *stream);
int lifeapi_symmetricize_offsets_batch_dev(const uint64_t *d_in, uint64_t *d_out, size_t n,
                                           uint32_t symmetry, const int32_t *d_offsets, void *stream);
/* d_out[u] = d_a[u].Convolve(d_b[u].Transformed(transform)) (LifeAPI.hpp:1293-1370,
 * Symmetry.hpp:105-173): both operands per universe, one SymmetryTransform
 * (0..15) per launch.  Convolve is symmetric in its operands; each universe's
 * sparser operand is walked, so the time is proportional to the smaller
 * population, and an empty operand gives the empty state.  d_b == d_a is the
 * self-convolution (each universe is read once); d_out may be d_a or d_b; any
 * other overlap is LIFEAPI_E_INVALID.                                       */
int lifeapi_convolve_pair_batch_dev(const uint64_t *d_a, const uint64_t *d_b, uint32_t transform,
                                    uint64_t *d_out, size_t n, void *stream);
/* d_out[u] = IntersectingOffsets(pat1[u], pat2[u], symmetry)  (Symmetry.hpp:729-768):
 * pat2.Convolve(pat1.Transformed(t)), t = Identity for C2, Rotate270 for C4, ReflectAcrossY for
 * D2AcrossX, ReflectAcrossX for D2AcrossY, ReflectAcrossYeqNegXP1 for D2diagodd, ReflectAcrossYeqX
 * for D2negdiagodd.  Every other symmetry (the reference's __builtin_unreachable, C1, D4 and
 * D4diag included) is LIFEAPI_E_INVALID.  d_pat2 == d_pat1 is IntersectingOffsets(active, sym)
 * (Symmetry.hpp:770-772).  Aliasing as lifeapi_convolve_pair_batch_dev.     */
int lifeapi_intersecting_offsets_batch_dev(const uint64_t *d_pat1, const uint64_t *d_pat2,
                                           uint32_t symmetry, uint64_t *d_out, size_t n, void *stream);
/* d_out[u] = d_in[u].Halve() (mode 0), HalveX() (1) or HalveY() (2)
 * (Symmetry.hpp:681-709): every second column and / or row, the half-size
 * result repeated in both halves.  Any other mode is LIFEAPI_E_INVALID.
 * d_out may be d_in.                                                        */
int lifeapi_halve_batch_dev(const uint64_t *d_in, uint64_t *d_out, size_t n, uint32_t mode, void *stream);
/* d_out[u] = d_in[u].Skew(), (x, y) -> (x, y + x) (Symmetry.hpp:711-718), or
 * with inverse != 0 InvSkew(), (x, y) -> (x, y - x) (Symmetry.hpp:720-727).
 * d_out may be d_in.                                                        */
int lifeapi_skew_batch_dev(const uint64_t *d_in, uint64_t *d_out, size_t n, int inverse, void *stream);
/* d_bounds[4u .. 4u+3] = d_states[u].XYBounds() (LifeAPI.hpp:446-484):
 * {left, top, right, bottom} in the window [-32, 31], -1 four times for an
 * empty state                                                              */
int lifeapi_bounds_batch_dev(const uint64_t *d_states, int32_t *d_bounds, size_t n, void *stream);
/* SymmetryOrbit / SymmetryOrbitRepresentatives (Symmetry.hpp:798-830).
 * d_images (may be NULL): n x 8 x 64 words, image i = Transformed(t_i) moved by
 *   minus its XYBounds' (left, top), t_i in the reference's order: Identity,
 *   ReflectAcrossX, ReflectAcrossYeqX, ReflectAcrossY, ReflectAcrossYeqNegXP1,
 *   Rotate90, Rotate270, Rotate180OddBoth.
 * d_first (may be NULL): bit i of d_first[u] is set iff image i equals no earlier
 *   image.  The set bits are the representatives; their images are SymmetryOrbit().
 * Both NULL is an error.  No output may overlap the input.                  */
int lifeapi_symmetry_orbit_batch_dev(const uint64_t *d_states, uint64_t *d_images, uint8_t *d_first,
                                     size_t n, void *stream);
/* d_cells[2u], d_cells[2u+1] = d_states[u].FirstOn() (LifeAPI.hpp:301-323), the
 * cell FirstCell() holds (LifeAPI.hpp:358) and Components() starts each piece
 * from: the LAST group of four columns (x = 0, 4, .., 60) that is not empty, in
 * it the lowest non-empty column, in that column the lowest set row; (-1, -1)
 * for the empty state.                                                      */
int lifeapi_first_on_batch_dev(const uint64_t *d_states, int32_t *d_cells, size_t n, void *stream);
/* d_out[u] = d_states[u].ComponentContaining(seed_u, corona) (LifeAPI.hpp:655-665):
 * with N(t) = t.Convolve(corona) & state, the least R with R = N(seed) | N(R).
 * So a seed cell outside the state is not in the result, a seed next to a
 * component returns that component, an empty seed or corona gives the empty
 * state, and a corona without (0, 0) may drop the seed.
 * d_seeds: 64 words (per_universe_seeds == 0, one seed for the batch) or n x 64.
 * corona: a HOST pointer to 64 words, read before the call returns; NULL = the
 *   reference's default b3o$5o$5o$5o$b3o! at (-2, -2) (LifeAPI.hpp:1185-1186).
 *   It is the one argument of a _dev call that is not a device pointer: it is
 *   checked before anything is launched and goes to the kernel by value, so
 *   the call owns no staging buffer whose lifetime a stream would have to
 *   guard.  The default corona, the 3 x 3 block and the 5-cell plus (centred)
 *   have networks of their own; any other corona costs time in proportion to
 *   its cells.
 * d_out may be d_states, or d_seeds when per-universe; any other overlap is
 * rejected.                                                                 */
int lifeapi_component_containing_batch_dev(const uint64_t *d_states, const uint64_t *d_seeds,
                                           int per_universe_seeds, const uint64_t *corona,
                                           uint64_t *d_out, size_t n, void *stream);
/* d_states[u].Components(corona) (LifeAPI.hpp:667-676): until nothing remains,
 * the component of FirstCell() of what remains, which is then removed.
 * corona: as above (a HOST pointer, NULL = the default).  It must contain cell
 *   (0, 0): without it the reference's loop never ends, and this call returns
 *   LIFEAPI_E_INVALID.
 * d_count (may be NULL): d_count[u] = the true number of components.
 * d_components (may be NULL): n x max_components x 64 words; component
 *   i < min(count, max_components) of universe u at ((u * max_components) + i) * 64,
 *   in the reference's order.  Slots from count up to max_components are not
 *   written.  A caller that needs every component asks for the counts first
 *   and sizes a second call by their maximum; one that expects few passes a
 *   small cap and reads count > cap as "truncated".
 * Both NULL, or d_components with max_components == 0, is an error.  No output
 * may overlap the input.                                                    */
int lifeapi_components_batch_dev(const uint64_t *d_states, const uint64_t *corona, uint32_t *d_count,
                                 uint64_t *d_components, uint32_t max_components, size_t n,
                                 void *stream);
/* Inclusive 3x3 neighbourhood count of each universe as 4 planes:
 * d_out = n x {bit3, bit2, bit1, bit0} x 64 words.
 * Replaces NeighbourCount(const LifeState&) (NeighbourCount.hpp:40-70) and
 * LifeState::CountNeighbourhood (LifeAPI.hpp:909-952).                    */
int lifeapi_neighbour_count_batch_dev(const uint64_t *d_in, uint64_t *d_out, size_t n, void *stream);
/* LifeState::InteractionCounts (LifeAPI.hpp:956-993): d_out = n x {out1,
 * out2, outMore} x 64 words; with_next != 0: InteractionCountsAndNext
 * (LifeAPI.hpp:997-1040), d_out = n x {out1, out2, outMore, next} x 64.     */
int lifeapi_interaction_counts_batch_dev(const uint64_t *d_in, uint64_t *d_out, size_t n,
                                         int with_next, void *stream);
/* LifeStable propagation passes, in place on LifeStable[n] = {state,
 * unknown, live2, live3, dead0, dead1, dead2, dead4, dead5, dead6} x 64
 * words (member order, LifeStable.hpp:41-53; option planes 1 = ruled out).
 * pass: 0 SynchroniseStateKnown (LifeStable.hpp:526-556), 1 UpdateOptions
 * (:558-615), 2 SignalNeighbours (:617-675), 3 PropagateStep (:695-716),
 * 4 Propagate (:718-729, at most max_iters steps; 0 = 2^20),
 * 5 StabiliseOptions (:677-693, the same bound); passes 0-3 ignore max_iters.
 * d_flags[u] = consistent | changed << 1, i.e. the PropagateResult; planes
 * are left exactly as the reference leaves them, including on an
 * inconsistent early return.  Where max_iters stopped 4 / 5 -- max_iters
 * iterations ran, none inconsistent, and the last one still changed
 * something -- d_flags[u] = 1 | 2 | 4 and the planes are the reference's
 * after exactly max_iters iterations.  That includes an object whose
 * max_iters-th iteration was the last to change anything: its planes are
 * the fixpoint's already, but the iteration that would confirm it has not
 * run; from max_iters + 1 on its flags are 1 | 2.  An iteration found
 * inconsistent within the bound gives 0, one that changes nothing 1 | 2 (or 1
 * if it was the first), whatever the bound.  Only the 128-byte lines
 * holding a changed column are written back (the rest is already there).  */
int lifeapi_stable_pass_batch_dev(uint64_t *d_planes, uint8_t *d_flags, size_t n, int pass,
                                  uint32_t max_iters, void *stream);
/* LifeStable::Vulnerable() (LifeStable.hpp:366-412) of every LifeStable[n]
 * (layout as above): d_out = n LifeStates.                                */
int lifeapi_stable_vulnerable_batch_dev(const uint64_t *d_planes, uint64_t *d_out, size_t n, void *stream);
/* The LifeStable lookahead family: one-cell lookahead and the strip passes it
 * is built from, in place on LifeStable[n] (layout of
 * lifeapi_stable_pass_batch_dev).  Every argument is checked before a device
 * is touched: null or misaligned d_planes / d_cells, null d_columns / d_flags,
 * d_cells, d_columns or d_flags overlapping d_planes and a pass outside 0..5
 * are LIFEAPI_E_INVALID; n == 0 succeeds with any pointers.
 *
 * Strip passes, each object at its own column d_columns[u] (0..63; the low six
 * bits are taken).
 * pass: 0 SynchroniseStateKnownStrip (LifeStable.hpp:921-948)
 *       1 UpdateOptionsStrip         (:1111-1195)
 *       2 SignalNeighboursStrip      (:995-1109)
 *       3 PropagateStepStrip         (:1215-1236)
 *       4 PropagateStrip             (:1238-1249)
 *       5 StabiliseOptionsStrip      (:1197-1213)
 * d_flags[u] is the reference's PropagateResult, consistent | changed << 1;
 * max_iters as lifeapi_stable_pass_batch_dev defines it (0 = 2^20; passes 0-3
 * ignore it; | 4 when the bound stopped 4 / 5, the planes then the reference's
 * after exactly max_iters iterations).  An inconsistent step or loop gives
 * {false, false} = 0; passes 0 and 1 report {abort == 0, changes != 0} as the
 * reference does, so 2 is possible there.  Planes are left exactly as the
 * reference leaves them, every inconsistent early return included, and the
 * strip passes differ from the full ones here: SynchroniseStateKnownStrip and
 * UpdateOptionsStrip finish all their columns and then report the abort,
 * SignalNeighboursStrip returns before writing, PropagateStepStrip stops at
 * the first inconsistent pass.  A strip pass reads columns x-2 .. x+3 of the
 * state and unknown planes and x-1 .. x+2 of the option planes (the torus),
 * and writes inside x-2 .. x+3: a strip propagation stops where a full one
 * would go on.                                                              */
int lifeapi_stable_strip_pass_batch_dev(uint64_t *d_planes, const uint8_t *d_columns, uint8_t *d_flags,
                                        size_t n, int pass, uint32_t max_iters, void *stream);
/* d_planes[u].TestUnknowns(cells_u) (LifeStable.hpp:1321-1338, TestUnknown
 * :1251-1284, Join :217-233), in place.  d_cells: 64 words (per_object_cells
 * == 0) or n x 64.  The cells are visited in FirstOn() order (LifeAPI.hpp:
 * 301-323) and what remains is narrowed by the new `unknown` after every
 * cell, as the reference does: the result depends on that order.  TestUnknown
 * with an inconsistent on-trial sets the cell off in the object itself and
 * propagates there; if that fails too the object is left so and the result is
 * {false, false}.
 * d_flags[u] = consistent | changed << 1 (inconsistent: 0).  max_iters (0 =
 * 2^20) bounds every PropagateStrip loop, each counted on its own; where it
 * stops one, d_flags[u] = 4 and object u is not written at all (a half-run
 * lookahead has no reference meaning).                                      */
int lifeapi_stable_test_unknowns_batch_dev(uint64_t *d_planes, const uint64_t *d_cells, int per_object_cells,
                                           uint8_t *d_flags, size_t n, uint32_t max_iters, void *stream);
/* d_planes[u].PropagateAndTest() (LifeStable.hpp:163-184), in place:
 * Propagate(), then TestUnknowns(Vulnerable().ZOI()), until neither changes.
 * d_flags as above.  max_iters (0 = 2^20) bounds every Propagate loop, every
 * PropagateStrip loop and the outer loop, each counted on its own; where it
 * stops any, d_flags[u] = 4 and object u is not written at all.             */
int lifeapi_stable_propagate_and_test_batch_dev(uint64_t *d_planes, uint8_t *d_flags, size_t n,
                                                uint32_t max_iters, void *stream);
/* d_planes[u].CompleteStable(minimise, useSeed, seed) (LifeStable.hpp:
 * 1340-1458): given the known part of a still life, find the rest, or prove
 * that there is none.  A backtracking search, one wave per object, its
 * recursion an explicit stack of frames in d_workspace.
 *
 * The reference's wall-clock timeout is a per-object node budget.  `nodes`
 * counts the entries of CompleteStableStep over the whole call, tail calls
 * (the on-branches) included, and "the clock is past the limit" is
 * nodes >= node_budget, tested where the reference reads the time: at the
 * entry of CompleteStableStep (:1343), before the node counts itself, so that
 * exactly node_budget nodes can run; and after each search-area round (:1439).
 * node_budget 0 = 1 << 16; above 1 << 24 is LIFEAPI_E_INVALID (one wave's
 * search must end).
 *
 * Everything else is the reference's, quirks included: maxPop and best carry
 * over between the rounds and into the minimise pass; a TIMEOUT with a
 * non-empty best is COMPLETED (:1444); a timeout inside the minimise pass is
 * ignored (:1450-1455); an empty state completes to the empty state and an
 * empty unknown to the state itself, searching nothing (:1415-1420); each round
 * masks the `unknown` plane alone; the branching cell is FirstOn of
 * Vulnerable() & settable, else of the settable cells whose NeighbourCount of
 * unknown is 2, else 3, else of settable (:1378-1391), FirstOn in the
 * reference's own order (the last populated group of four columns); the
 * pruning is currentPop >= maxPop (:1353).
 *
 * Three cases the reference leaves undefined are defined here:
 *   - unknown within state.ZOI() at the start (no round would run, :1432, and
 *     `result` be read uninitialised): CompleteStableStep runs once on the
 *     object as given, its unknown plane unmasked, and the call goes on from
 *     that result (searchArea = state.ZOI() for the minimise pass);
 *   - LIFEAPI_COMPLETE_USE_SEED with an empty seed (the loop at :1369 would
 *     not end): result 4, best empty, nothing searched -- after the two early
 *     returns above, which do not look at the seed;
 *   - a search that needs more than max_depth frames: result 3, best empty.
 *
 * d_result[u]: 0 COMPLETED, 1 INCONSISTENT, 2 TIMEOUT (the reference's enum
 * order), 3 too deep, 4 bad seed.  d_best[u]: the completion, the empty state
 * unless COMPLETED.  d_nodes (may be NULL): the nodes entered.  d_planes is
 * not written.  d_seeds: one LifeState (per_object_seeds 0) or n; ignored
 * without LIFEAPI_COMPLETE_USE_SEED.
 *
 * d_workspace (128-byte aligned) holds a 256-byte header and one stack of
 * max_depth frames of 5376 bytes (the 10 planes and the cell) per resident
 * wave, not per object: the waves claim their objects from a counter in the
 * header.  lifeapi_stable_complete_workspace_bytes(n, max_depth) is what a
 * full grid for n objects uses on the current device (0, with
 * lifeapi_last_error(), if there is none or max_depth is invalid); any size
 * that holds the header and one stack is accepted and only lowers the number
 * of concurrent searches.  The call clears the header on `stream`.
 *
 * LIFEAPI_E_INVALID: null or misaligned pointers, outputs overlapping inputs,
 * each other or the workspace, a workspace below one stack, unknown flag
 * bits, USE_SEED with a null seed, max_depth 0 or above 4096, a budget above
 * 1 << 24.  n == 0 succeeds with any pointers.                              */
#define LIFEAPI_COMPLETE_MINIMISE 1u
#define LIFEAPI_COMPLETE_USE_SEED 2u
size_t lifeapi_stable_complete_workspace_bytes(size_t n, uint32_t max_depth);
int lifeapi_stable_complete_batch_dev(const uint64_t *d_planes, const uint64_t *d_seeds, int per_object_seeds,
                                      uint32_t flags, uint64_t node_budget, uint32_t max_depth, uint64_t *d_best,
                                      uint8_t *d_result, uint64_t *d_nodes, size_t n, void *d_workspace,
                                      size_t workspace_bytes, void *stream);
/* LifeWeld::Step() (LifeWeld.hpp:169-186) `generations` times, in place on
 * LifeWeld[n] = {state, frozen2, frozen1, frozen0} x 64 words (the struct's
 * member order, LifeWeld.hpp:18-20); only the state planes change.        */
int lifeapi_weld_step_batch_dev(uint64_t *d_welds, size_t n, uint32_t generations, void *stream);
/* The LifeWeld construction family.  LifeWeld[n] and LifeStable[n] in the
 * layouts above; every function is defined for any bit patterns (frozen counts
 * on live cells, a `required` unrelated to the state, an `active` over the
 * state).  No output may overlap an input or another output.
 *
 * d_welds[u] = LifeWeld::FromRequired(d_states[u], required_u) (LifeWeld.hpp:
 * 133-159).  d_required: 64 words (per_universe_required == 0) or n x 64.   */
int lifeapi_weld_from_required_batch_dev(const uint64_t *d_states, const uint64_t *d_required,
                                         int per_universe_required, uint64_t *d_welds, size_t n,
                                         void *stream);
/* (d_wanted[u], d_unwanted[u]) = d_welds[u].ToTarget() (LifeWeld.hpp:188-191),
 * the halves of a LifeTarget, n x 64 words each.                            */
int lifeapi_weld_to_target_batch_dev(const uint64_t *d_welds, uint64_t *d_wanted, uint64_t *d_unwanted,
                                     size_t n, void *stream);
/* d_stables[u] = d_welds[u].ToStable(active_u, duration, mask) (LifeWeld.hpp:
 * 279-400), ready for lifeapi_stable_pass_batch_dev.
 * d_active: NULL (the empty state), 64 words (per_universe_active == 0) or
 *   n x 64.  d_mask: NULL (= ~LifeState(), the reference's default) or 64 words.
 * duration == 0 is exactly ToStable() (LifeWeld.hpp:279-325), whatever active
 * and mask are.  duration > 65536 is LIFEAPI_E_INVALID (a bound on one
 * launch's time, which grows in proportion to duration; a reaction that
 * reaches a fixed point stops costing there).                               */
int lifeapi_weld_to_stable_batch_dev(const uint64_t *d_welds, const uint64_t *d_active,
                                     int per_universe_active, const uint64_t *d_mask, uint32_t duration,
                                     uint64_t *d_stables, size_t n, void *stream);
/* d_out[u] = d_welds[u].InteractionOffsets(other) (LifeWeld.hpp:206-245):
 * LifeState::InteractionOffsets with every plane but the overlap term's
 * masked by its side's (state & ~frozen2 & ~frozen1 & ~frozen0).ZOI() -- except
 * that, as in the reference (LifeWeld.hpp:238-239), the second operand of
 * each birth term is masked by the FIRST operand's side.
 * d_other: one LifeWeld, 256 words.                                         */
int lifeapi_weld_interaction_offsets_batch_dev(const uint64_t *d_welds, const uint64_t *d_other,
                                               uint64_t *d_out, size_t n, void *stream);
/* Config-5 ternary step: bitslicing/unknown_step_refined.hpp:1-85 applied
 * per column with s2..s0 / on2..on0 = bits 2..0 of NeighbourCount
 * (NeighbourCount.hpp:40-70) of stable.state / current.state.
 * d_in: n x 11 planes x 64 words (stable.state, current.state,
 * current.unknown, live2, live3, dead0, dead1, dead2, dead4, dead5, dead6;
 * option planes 1 = ruled out, LifeStable.hpp:41-53).  d_out: n x 3 planes
 * (next_on, next_unknown, next_unknown_stable).  No overlap allowed.      */
int lifeapi_refined_step_batch_dev(const uint64_t *d_in, uint64_t *d_out, size_t n, void *stream);
/* synthetic universes: word w = u*64+x (u counted from first_universe) is
 * splitmix64(seed + (w+1)*0x9E3779B97F4A7C15); mode 1 maps each column to
 * [2^61, 2^62) like RandomState()                                         */
int lifeapi_fill_random_dev(uint64_t *d_out, size_t n, uint64_t seed,
                            uint64_t first_universe, int mode, void *stream);
/* RLE batch I/O.  Text is a byte blob; pattern u is bytes
 * [offsets[u], offsets[u+1]) (n+1 offsets, no terminators).
 * LifeState::RLE() (Parsing.hpp:8-63,200-204; rows and columns printed
 * from 32, as the reference does): lengths first, the caller scans them
 * into offsets, then the write.                                           */
int lifeapi_rle_lengths_batch_dev(const uint64_t *d_states, uint32_t *d_len, size_t n, void *stream);
int lifeapi_rle_write_batch_dev(const uint64_t *d_states, const uint64_t *d_offsets, char *d_text,
                                size_t n, void *stream);
/* LifeState::Parse (GenericParse, Parsing.hpp:143-198) of every pattern.
 * d_status[u] bit 0: a live cell off the 64x64 board was dropped (the
 * reference writes out of bounds there); bit 1: parsing stopped at a "$"
 * count of 129 (the reference's early return, Parsing.hpp:171-173).       */
int lifeapi_parse_rle_batch_dev(const char *d_text, const uint64_t *d_offsets, size_t n,
                                uint64_t *d_out, uint8_t *d_status, void *stream);

/* ---- host pointers, synchronous ----------------------------------------- */

/* Stages through device memory of `device` (or of every visible device,
 * contiguous shards, one host thread each, when device == -1; the
 * environment variable LIFEAPI_HOST_SHARDS=k overrides that shard count,
 * shard s running on device s mod count -- a rehearsal knob for machines
 * with fewer GPUs).                                                        */
int lifeapi_step_batch(const uint64_t *in, uint64_t *out, size_t n, uint32_t generations,
                       int device);
int lifeapi_pop_batch(const uint64_t *states, uint32_t *pop, size_t n, int device);
/* host-pointer forms of the *_dev entry points above (same layouts); each
 * stages through `device` in chunks of <= 64 MiB per array, two chunks in
 * flight (one per direction of the link); device -1 shards over every
 * visible device as above                                                 */
int lifeapi_weld_step_batch(uint64_t *welds, size_t n, uint32_t generations, int device);
int lifeapi_stable_pass_batch(uint64_t *planes, uint8_t *flags, size_t n, int pass,
                              uint32_t max_iters, int device);
int lifeapi_stable_vulnerable_batch(const uint64_t *planes, uint64_t *out, size_t n, int device);
int lifeapi_neighbour_count_batch(const uint64_t *in, uint64_t *out, size_t n, int device);
int lifeapi_interaction_counts_batch(const uint64_t *in, uint64_t *out, size_t n, int with_next,
                                     int device);
int lifeapi_refined_step_batch(const uint64_t *in, uint64_t *out, size_t n, int device);
int lifeapi_contains_batch(const uint64_t *states, const uint64_t *wanted, const uint64_t *unwanted,
                           uint8_t *out, size_t n, int device);
/* host forms of the per-offset entry points: out (may equal states) and
 * count as the *_dev forms take them (lifeapi_match_batch: one may be NULL) */
int lifeapi_match_batch(const uint64_t *states, const uint64_t *wanted, const uint64_t *unwanted,
                        uint64_t *out, uint32_t *count, size_t n, int device);
int lifeapi_convolve_batch(const uint64_t *states, const uint64_t *pattern, uint64_t *out, size_t n,
                           int device);
int lifeapi_interaction_offsets_batch(const uint64_t *states, const uint64_t *other, uint64_t *out,
                                      size_t n, int device);
/* host forms of the symmetry entry points: out may equal in; images and
 * first as lifeapi_symmetry_orbit_batch_dev takes them (one may be NULL)   */
int lifeapi_transform_batch(const uint64_t *in, uint64_t *out, size_t n, uint32_t transform, int dx, int dy,
                            int device);
int lifeapi_symmetricize_batch(const uint64_t *in, uint64_t *out, size_t n, uint32_t symmetry, int dx,
                               int dy, int device);
/* (offsets: n x {dx, dy} int32 on the host; a, b and out of the pair calls
 * alias as the *_dev forms allow)                                          */
int lifeapi_transform_offsets_batch(const uint64_t *in, uint64_t *out, size_t n, uint32_t transform,
                                    const int32_t *offsets, int device);
int lifeapi_symmetricize_offsets_batch(const uint64_t *in, uint64_t *out, size_t n, uint32_t symmetry,
                                       const int32_t *offsets, int device);
int lifeapi_convolve_pair_batch(const uint64_t *a, const uint64_t *b, uint32_t transform, uint64_t *out,
                                size_t n, int device);
int lifeapi_intersecting_offsets_batch(const uint64_t *pat1, const uint64_t *pat2, uint32_t symmetry,
                                       uint64_t *out, size_t n, int device);
int lifeapi_halve_batch(const uint64_t *in, uint64_t *out, size_t n, uint32_t mode, int device);
int lifeapi_skew_batch(const uint64_t *in, uint64_t *out, size_t n, int inverse, int device);
int lifeapi_bounds_batch(const uint64_t *states, int32_t *bounds, size_t n, int device);
int lifeapi_symmetry_orbit_batch(const uint64_t *states, uint64_t *images, uint8_t *first, size_t n,
                                 int device);
/* host forms of the connected-component entry points: the same arguments
 * (corona a host pointer there too); out may equal states, or seeds when
 * per-universe; components is read as well as written, so that the slots past
 * a universe's count keep the caller's bytes                                */
int lifeapi_first_on_batch(const uint64_t *states, int32_t *cells, size_t n, int device);
int lifeapi_component_containing_batch(const uint64_t *states, const uint64_t *seeds,
                                       int per_universe_seeds, const uint64_t *corona, uint64_t *out,
                                       size_t n, int device);
int lifeapi_components_batch(const uint64_t *states, const uint64_t *corona, uint32_t *count,
                             uint64_t *components, uint32_t max_components, size_t n, int device);
/* host forms of the LifeWeld construction entry points: the same arguments
 * and the same overlap rules, on host arrays                                */
int lifeapi_weld_from_required_batch(const uint64_t *states, const uint64_t *required,
                                     int per_universe_required, uint64_t *welds, size_t n, int device);
int lifeapi_weld_to_target_batch(const uint64_t *welds, uint64_t *wanted, uint64_t *unwanted, size_t n,
                                 int device);
int lifeapi_weld_to_stable_batch(const uint64_t *welds, const uint64_t *active, int per_universe_active,
                                 const uint64_t *mask, uint32_t duration, uint64_t *stables, size_t n,
                                 int device);
int lifeapi_weld_interaction_offsets_batch(const uint64_t *welds, const uint64_t *other, uint64_t *out,
                                           size_t n, int device);
/* host forms of the LifeStable lookahead entry points: the same arguments and
 * the same checks, on host arrays                                           */
int lifeapi_stable_strip_pass_batch(uint64_t *planes, const uint8_t *columns, uint8_t *flags, size_t n,
                                    int pass, uint32_t max_iters, int device);
int lifeapi_stable_test_unknowns_batch(uint64_t *planes, const uint64_t *cells, int per_object_cells,
                                       uint8_t *flags, size_t n, uint32_t max_iters, int device);
int lifeapi_stable_propagate_and_test_batch(uint64_t *planes, uint8_t *flags, size_t n, uint32_t max_iters,
                                            int device);
/* host form of lifeapi_stable_complete_batch_dev: the same arguments and
 * checks on host arrays; it allocates its own workspace (at most 1 GiB per
 * staging stream, kept for the process)                                     */
int lifeapi_stable_complete_batch(const uint64_t *planes, const uint64_t *seeds, int per_object_seeds, uint32_t flags,
                                  uint64_t node_budget, uint32_t max_depth, uint64_t *best, uint8_t *result,
                                  uint64_t *nodes, size_t n, int device);
/* host form of lifeapi_step_contains_batch_dev: the search-loop idiom
 * "for g in 1..gens: s.Step(); if (s.Contains(target)) ..." (LifeAPI.hpp:
 * 1196-1216, LifeTarget.hpp:44-51) over n host universes; final (may be NULL,
 * may equal in) receives Stepped(gens); device -1 shards the batch over all
 * visible GPUs as lifeapi_step_batch does                                  */
int lifeapi_step_contains_batch(const uint64_t *in, uint64_t *final_states, const uint64_t *wanted,
                                const uint64_t *unwanted, uint32_t *first_gen, size_t n,
                                uint32_t generations, int device);
/* RLE of every state: fills offsets[0..n] (offsets[n] = total bytes); with
 * text == NULL only the offsets (size query), else writes the patterns to
 * text (LIFEAPI_E_INVALID if text_cap < offsets[n])                       */
int lifeapi_rle_batch(const uint64_t *states, size_t n, char *text, size_t text_cap, uint64_t *offsets,
                      int device);
int lifeapi_parse_rle_batch(const char *text, const uint64_t *offsets, size_t n, uint64_t *out,
                            uint8_t *status, int device);

/* Page-lock a host array the caller reuses across calls (hipHostRegister,
 * portable to every device).  The host-pointer entry points move page-locked
 * memory by DMA in both directions at once (about 97 GB/s combined against
 * 56 GB/s for pageable memory, profiles/r01/host_bench.jsonl).  A call moving
 * at least 8 MiB pins pageable arrays itself for its duration, so this is
 * optional: it holds the pin across calls, and covers smaller calls.
 * Unregister before freeing the memory, and do not register or unregister
 * an array while another thread's call on it is in flight (the per-call
 * pins are counted across threads; the runtime does not count
 * registrations).  New in this build: the reference has no host/device
 * split at all.                                                            */
int lifeapi_host_register(void *p, size_t bytes);
int lifeapi_host_unregister(void *p);

#ifdef __cplusplus
}
#endif
#endif /* LIFEAPI_HIP_H */
