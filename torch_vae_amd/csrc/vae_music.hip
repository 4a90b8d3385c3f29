// The per-roll musical statistics of the C ABI (include/vae_music.h; kernels in music_stats.cuh).  Context-free, like vae_util.hip;
// no work space, nothing is read back and nothing waits for the device.
#include "vae_ctx.h"
#include "../../include/vae_music.h"
#include "music_stats.cuh"

static_assert(MS_FEATURES == VAE_MUSIC_FEATURES, "music_stats.cuh and include/vae_music.h disagree on the feature row");

extern "C" int vae_music_roll_stats(const uint8_t* planes, int64_t n, int h, int w, int pitch_offset, int32_t* features, int64_t* totals,
                                    int accumulate, vae_stream_t stream) {
    const char* what = "vae_music_roll_stats";
    if (!planes || !features) return vae_set_error(what, "null pointer (planes, features)");
    if (n < 0) return vae_set_error(what, "n must be >= 0");
    if (h < 1) return vae_set_error(what, "h must be >= 1");
    if (w < 32 || w % 32) return vae_set_error(what, "w must be a positive multiple of 32");
    if ((int64_t)h * (w / 8) > MS_MAX_ROLL_BYTES) return vae_set_error(what, "a roll (h * w / 8 bytes) must fit 8192 bytes");
    if (pitch_offset < 0 || pitch_offset > (1 << 20)) return vae_set_error(what, "pitch_offset must be in 0..2^20");
    if (n > ((int64_t)1 << 40) / MS_FEATURES) return vae_set_error(what, "n * 76 features must stay within 2^40");
    if ((reinterpret_cast<uintptr_t>(planes) | reinterpret_cast<uintptr_t>(features)) & 3) return vae_set_error(what, "planes and features must be 4-byte aligned");
    if (reinterpret_cast<uintptr_t>(totals) & 7) return vae_set_error(what, "totals must be 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    long long* tot = reinterpret_cast<long long*>(totals);
    if (tot && !accumulate && launch("music_totals_init_kernel", music_totals_init_kernel, dim3(1), dim3(128), 0, st, tot)) return -1;
    if (n == 0) return 0;
    const int wd = w / 32;
    int shift = -1;
    if ((wd & (wd - 1)) == 0) for (shift = 0; (1 << shift) < wd; ++shift) {}
    MusicArgs a{reinterpret_cast<const unsigned*>(planes), (long)n, h, wd, shift, pitch_offset, features};
    const size_t lds = (size_t)MS_WAVES * ms_wave_words(h, wd) * sizeof(unsigned);
    const long blocks = (long)((n + MS_WAVES - 1) / MS_WAVES);
    if (launch("music_roll_stats_kernel", music_roll_stats_kernel, dim3((unsigned)std::min<long>(blocks, MS_MAX_BLOCKS)), dim3(64 * MS_WAVES), lds, st, a)) return -1;
    if (!tot) return 0;
    const long tblocks = (long)((n + MS_TOTAL_ROLLS - 1) / MS_TOTAL_ROLLS);
    return launch("music_totals_kernel", music_totals_kernel, dim3((unsigned)std::min<long>(tblocks, 4096)), dim3(256), 0, st, (const int*)features, (long)n, tot);
}
