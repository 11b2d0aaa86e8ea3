// The reference's frame loop from C++ (Content/Voxelizer.cpp:81-113, :371-399, through include/dxv_voxelizer.hpp): three frames in
// flight, each with its own camera and its own render target on the GPU --
//   SetViewport(width, height);  for i in 0 .. 5: UpdateFrame(i % 3, eye, viewProj); Render(i % 3, gridDim, target[i % 3], pitch);
//   then ONE wait for all frames.
// usage: render_loop verts.bin indices.bin cameras.bin gridDim width height out_prefix
//   verts.bin: numVerts x 6 floats, indices.bin: 3 x numTris uint32, cameras.bin: 3 x (eye[3], viewProj[16]) floats.
// Writes the three frames' last images to out_prefix0.bin .. out_prefix2.bin (height x width x 4 bytes each).
#include "../../include/dxv_voxelizer.hpp"

#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

template <class T>
static bool readAll(const char* path, std::vector<T>& out)
{
	FILE* f = fopen(path, "rb");
	if (!f) return false;
	fseek(f, 0, SEEK_END);
	const long bytes = ftell(f);
	fseek(f, 0, SEEK_SET);
	out.resize(static_cast<size_t>(bytes) / sizeof(T));
	const bool ok = fread(out.data(), sizeof(T), out.size(), f) == out.size();
	fclose(f);
	return ok;
}

int main(int argc, char** argv)
{
	if (argc < 8) { fprintf(stderr, "usage: %s verts.bin indices.bin cameras.bin gridDim width height out_prefix\n", argv[0]); return 2; }
	std::vector<float> vb, cams;
	std::vector<uint32_t> ib;
	if (!readAll(argv[1], vb) || !readAll(argv[2], ib) || !readAll(argv[3], cams) || cams.size() != 3 * 19) {
		fprintf(stderr, "cannot read the input files\n");
		return 2;
	}
	const uint32_t gridDim = static_cast<uint32_t>(atoi(argv[4]));
	const uint32_t width = static_cast<uint32_t>(atoi(argv[5])), height = static_cast<uint32_t>(atoi(argv[6]));
	const size_t pitch = static_cast<size_t>(width) * 4, bytes = pitch * height;
	Voxelizer voxelizer;
	if (!voxelizer.InitFromArrays(vb.data(), static_cast<uint32_t>(vb.size() / 6), ib.data(), static_cast<uint32_t>(ib.size() / 3), nullptr, false, gridDim)) {
		fprintf(stderr, "Init failed: %s\n", voxelizer.LastError());
		return 1;
	}
	voxelizer.SetViewport(width, height);
	void* targets[Voxelizer::FrameCount] = {};
	for (auto& t : targets)
		if (hipMalloc(&t, bytes) != hipSuccess) { fprintf(stderr, "hipMalloc failed\n"); return 1; }
	for (int i = 0; i < 6; ++i) {
		const uint8_t frame = static_cast<uint8_t>(i % Voxelizer::FrameCount);
		const float* cam = cams.data() + 19 * frame;
		if (!voxelizer.UpdateFrame(frame, cam, cam + 3)) { fprintf(stderr, "UpdateFrame failed: %s\n", voxelizer.LastError()); return 1; }
		if (!voxelizer.Render(frame, gridDim, targets[frame], pitch)) { fprintf(stderr, "Render failed: %s\n", voxelizer.LastError()); return 1; }
	}
	if (!voxelizer.WaitAll()) { fprintf(stderr, "WaitAll failed: %s\n", voxelizer.LastError()); return 1; }
	std::vector<uint8_t> image(bytes);
	for (int frame = 0; frame < Voxelizer::FrameCount; ++frame) {
		if (hipMemcpy(image.data(), targets[frame], bytes, hipMemcpyDeviceToHost) != hipSuccess) { fprintf(stderr, "hipMemcpy failed\n"); return 1; }
		const std::string path = std::string(argv[7]) + std::to_string(frame) + ".bin";
		FILE* f = fopen(path.c_str(), "wb");
		if (!f || fwrite(image.data(), 1, bytes, f) != bytes) { fprintf(stderr, "cannot write %s\n", path.c_str()); return 1; }
		fclose(f);
	}
	for (auto& t : targets) (void)hipFree(t);
	dxv_stats st{};
	voxelizer.GetStats(st);
	printf("%u %.4f\n", st.grid_dim, st.render_ms);
	return 0;
}
