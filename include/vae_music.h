/* C ABI of the per-roll musical statistics (libvae_step_gfx950.so, beside include/vae_step.h): what a set of pianorolls looks like
 * as music - notes, pitch classes, note lengths, polyphony, rhythm - counted on the device from bit planes, so that a set of
 * generated rolls can be held against the training set (Yang & Lerch 2020; the MuseGAN metrics of Dong et al. 2018).
 *
 * Conventions and the stream contract are those of vae_step.h: plain device pointers owned by the caller, work ordered on the
 * explicit stream (the last argument), nothing read back, 0 on success or -1 with the message in vae_last_error().  The entry
 * point never synchronises with the host and needs no work space.  Every output is an integer count, so no bit depends on the
 * order in which workgroups arrive and repeated calls give identical bits.
 */
#ifndef VAE_MUSIC_H
#define VAE_MUSIC_H
#include <stdint.h>
#include "vae_step.h"
#ifdef __cplusplus
extern "C" {
#endif

#define VAE_MUSIC_FEATURES 76

/* Statistics of n rolls given as bit planes [n][h][w/8]: h pitch rows by w time columns, most significant bit first
 * (numpy.packbits order) - the kind-1 source of vae_gather_rolls, the cleaned planes of vae_extract_notes, the planes of
 * vae_nearest_rolls.
 *
 * A CELL is a set bit.  A NOTE is a maximal run of set bits along time within one row; a run that starts at t = 0 or ends at
 * t = w-1 is a note like any other.  An ONSET is a note's first cell.  The PITCH CLASS of row p is (p + pitch_offset) mod 12.
 *
 * features [n][VAE_MUSIC_FEATURES] int32, for roll r:
 *    0       rolls            1
 *    1       nonempty         1 if cells > 0, else 0
 *    2       cells            popcount of the roll
 *    3       notes            number of notes
 *    4       used_pitches     rows with at least one cell
 *    5, 6    lowest, highest  the smallest / largest used row; -1, -1 for an empty roll
 *    7       sounding_steps   columns with at least one cell
 *    8       onset_steps      columns with at least one onset
 *    9       max_polyphony    the largest number of cells in one column
 *   10..21   pc_cells[12]     cells per pitch class
 *   22..33   pc_notes[12]     notes per pitch class
 *   34..45   duration[12]     notes of length len in bucket min(floor(log2 len), 11)
 *   46..61   polyphony[16]    columns with exactly k cells, k = 0..14; bucket 15 holds k >= 15
 *   62..73   ioi[12]          gaps g > 0 between consecutive onset steps in bucket min(floor(log2 g), 11)
 *   74, 75   reserved         0
 *
 * totals [VAE_MUSIC_FEATURES] int64, or null: over all n rolls the sum of every column - except `lowest`: the minimum over the
 * non-empty rolls, -1 if there is none; `highest` and `max_polyphony`: the maximum (-1 / 0 if there is none).  With
 * accumulate != 0 the call combines by the same rules with what totals already holds (an earlier `lowest` of -1 means "none
 * yet"); with accumulate == 0 it overwrites.
 *
 * n == 0 returns 0 and launches nothing, except that with accumulate == 0 a given totals is set to the empty value: zeros,
 * lowest -1, highest -1.  No byte outside planes, features and totals is addressed.
 *
 * Refused with -1 and "vae_music_roll_stats: <reason>" before anything is enqueued: null planes or features; n < 0; h < 1;
 * w not a positive multiple of 32; a roll of more than 8192 bytes (h * w / 8; the limit of vae_nearest_rolls, 256x256 fits);
 * pitch_offset outside 0..2^20; n * VAE_MUSIC_FEATURES beyond 2^40; planes or features not 4-byte aligned, totals not 8-byte
 * aligned. */
int vae_music_roll_stats(const uint8_t* planes, int64_t n, int h, int w, int pitch_offset, int32_t* features, int64_t* totals,
                         int accumulate, vae_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
