// chunk_stats_check.cpp -- the routines every reader of chunk sums shares (raytracing-rust_amd/csrc/rt_chunk_stats.h) run on the
// host, for tests/test_chunk_stats_host.py to compare with tests/noise_checker.py and tests/adaptive_checker.py bit for bit.  What
// the kernels call is what runs here: on the host the operators are the plain IEEE ones, so this checks the ARITHMETIC AS WRITTEN
// (order of operations, the clamp, the two sums, the state step in both of its forms) and both maps to a pixel.  Built by the test
// with `hipcc --cuda-host-only -ffp-contract=off -fno-fast-math -fsanitize=address,undefined`.
//
//   chunk_stats_check stats IN OUT
//     IN   u32 n_px, split, chunk_passes, has_albedo, keep_state, per_pixel_nb, n_batches; then albedo[n_px][3] f32 if has_albedo;
//          then per batch: sums[split][n_px][3] f32, mean_in[n_px][3] f32, mask[n_px] u32
//     OUT  per batch: lbar[n_px], var[n_px], out_mean[n_px][3], out_lum[n_px], out_var[n_px] f32 -- the planes as they stand after
//          the batch.  Batch 0 is fresh.  per_pixel_nb 0: every batch takes every pixel, the divisor is the batch number, the step
//          is the one with optional state and outputs (keep_state 0: one batch, no state; the variance plane is then not asked
//          for and stays +0).  per_pixel_nb 1: batches after the first take the masked pixels only, each divided by its own count.
//   chunk_stats_check maps W H TILE_W TILE_H OUT
//     OUT  i32: for every tile of the 8 x 8 grid and place 0..63 (inside, x, y); then for every work item of the TILE_W x TILE_H
//          render tiling the pixel index, or -1 for padding
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../raytracing-rust_amd/csrc/rt_chunk_stats.h"

template <class T> static std::vector<T> read_n(std::FILE *f, size_t n)
{
	std::vector<T> v(n);
	if (n && std::fread(v.data(), sizeof(T), n, f) != n) {
		std::fprintf(stderr, "short input\n");
		std::exit(1);
	}
	return v;
}
template <class T> static void write_v(std::FILE *f, const std::vector<T> &v)
{
	if (!v.empty() && std::fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) {
		std::fprintf(stderr, "cannot write\n");
		std::exit(1);
	}
}

static int stats(const char *in_path, const char *out_path)
{
	std::FILE *in = std::fopen(in_path, "rb"), *out = std::fopen(out_path, "wb");
	if (!in || !out)
		return 1;
	const std::vector<uint32_t> h = read_n<uint32_t>(in, 7);
	const uint32_t n_px = h[0], split = h[1], chunk_passes = h[2], has_albedo = h[3], keep_state = h[4], per_pixel_nb = h[5], n_batches = h[6];
	const std::vector<float> albedo = read_n<float>(in, has_albedo ? 3u * (size_t)n_px : 0u);
	std::vector<float> state_m(3u * (size_t)n_px), state_l(n_px), state_v(n_px), out_mean(3u * (size_t)n_px), out_lum(n_px), out_var(n_px);
	std::vector<uint32_t> count(n_px, 0u);
	for (uint32_t b = 0; b < n_batches; ++b) {
		const std::vector<float> sums = read_n<float>(in, 3u * (size_t)split * n_px), mean_in = read_n<float>(in, 3u * (size_t)n_px);
		const std::vector<uint32_t> mask = read_n<uint32_t>(in, n_px);
		std::vector<float> lbar(n_px), var(n_px);
		for (uint32_t p = 0; p < n_px; ++p) {
			const rt::Demod d = rt::demod_divisors(has_albedo ? albedo.data() : nullptr, 3u * (size_t)p);
			const rt::ChunkStats s = rt::chunk_stats(sums.data() + 3u * (size_t)p, 3u * (size_t)n_px, split, (float)chunk_passes, d);
			lbar[p] = s.lbar;
			var[p] = s.var;
			if (!per_pixel_nb || b == 0u) // as noise_chunk_kernel calls it
				rt::chunk_state_step<true>(p, mean_in.data(), s, keep_state ? state_m.data() : nullptr, state_l.data(), state_v.data(), b == 0u,
				                           (float)(b + 1u), out_mean.data(), out_lum.data(), keep_state ? out_var.data() : nullptr);
			else if (mask[p]) // as adaptive_fold_kernel calls it
				rt::chunk_state_step<false>(p, mean_in.data(), s, state_m.data(), state_l.data(), state_v.data(), false, (float)(count[p] + 1u),
				                            out_mean.data(), out_lum.data(), out_var.data());
			if (!per_pixel_nb || b == 0u || mask[p])
				count[p] += 1u;
		}
		write_v(out, lbar);
		write_v(out, var);
		write_v(out, out_mean);
		write_v(out, out_lum);
		write_v(out, out_var);
	}
	std::fclose(in);
	return std::fclose(out) != 0;
}

static int maps(uint32_t w, uint32_t h, uint32_t tile_w, uint32_t tile_h, const char *out_path)
{
	std::FILE *out = std::fopen(out_path, "wb");
	if (!out)
		return 1;
	std::vector<int32_t> v;
	const uint32_t tiles_x = (w + 7u) / 8u, tiles_y = (h + 7u) / 8u;
	for (uint32_t tile = 0; tile < tiles_x * tiles_y; ++tile)
		for (uint32_t place = 0; place < 64u; ++place) {
			uint32_t x = 0, y = 0;
			const bool inside = rt::grid8_pixel(tile, place, tiles_x, w, h, x, y);
			v.insert(v.end(), {(int32_t)inside, (int32_t)x, (int32_t)y});
		}
	const uint32_t across = (w + tile_w - 1u) / tile_w, down = (h + tile_h - 1u) / tile_h;
	for (uint32_t wp = 0; wp < across * down * tile_w * tile_h; ++wp) {
		size_t p = 0;
		v.push_back(rt::frame_work_pixel(wp, tile_w, tile_h, across, w, h, p) ? (int32_t)p : -1);
	}
	write_v(out, v);
	return std::fclose(out) != 0;
}

int main(int argc, char **argv)
{
	if (argc == 4 && argv[1][0] == 's')
		return stats(argv[2], argv[3]);
	if (argc == 7 && argv[1][0] == 'm')
		return maps((uint32_t)std::atoi(argv[2]), (uint32_t)std::atoi(argv[3]), (uint32_t)std::atoi(argv[4]), (uint32_t)std::atoi(argv[5]), argv[6]);
	std::fprintf(stderr, "usage: chunk_stats_check stats IN OUT | maps W H TILE_W TILE_H OUT\n");
	return 2;
}
