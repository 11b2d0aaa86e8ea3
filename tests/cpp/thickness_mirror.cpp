// The local thickness through the host-side C++ mirror include/dxv_voxelizer.hpp: InitFromArrays, Voxelize, Thickness for both kinds, then the map
// and the histogram.  Writes the solid map; prints, per kind, the members, the largest value, the minimum wall and the thickness in voxels there.
#include "../../include/dxv_voxelizer.hpp"

#include <cstdio>
#include <cstdlib>
#include <vector>

static std::vector<uint8_t> read_file(const char* path)
{
	std::vector<uint8_t> out;
	FILE* f = fopen(path, "rb");
	if (!f) return out;
	fseek(f, 0, SEEK_END);
	out.resize(static_cast<size_t>(ftell(f)));
	fseek(f, 0, SEEK_SET);
	if (fread(out.data(), 1, out.size(), f) != out.size()) out.clear();
	fclose(f);
	return out;
}

int main(int argc, char** argv)
{
	if (argc < 6) { fprintf(stderr, "usage: %s vb.bin ib.bin gridDim capSq map.bin\n", argv[0]); return 2; }
	const std::vector<uint8_t> vb = read_file(argv[1]), ib = read_file(argv[2]);
	if (vb.empty() || ib.empty()) { fprintf(stderr, "cannot read the mesh\n"); return 1; }
	const uint32_t gridDim = static_cast<uint32_t>(atoi(argv[3])), capSq = static_cast<uint32_t>(atoi(argv[4]));
	Voxelizer voxelizer;
	if (!voxelizer.InitFromArrays(reinterpret_cast<const float*>(vb.data()), static_cast<uint32_t>(vb.size() / 24),
		reinterpret_cast<const uint32_t*>(ib.data()), static_cast<uint32_t>(ib.size() / 12)))
	{ fprintf(stderr, "Init failed: %s\n", voxelizer.LastError()); return 1; }
	std::vector<uint32_t> field;
	std::vector<uint64_t> histogram;
	if (voxelizer.ThicknessField(field)) { fprintf(stderr, "a map before the first launch\n"); return 1; }
	if (!voxelizer.Voxelize(gridDim, Voxelizer::REFERENCE)) { fprintf(stderr, "Voxelize: %s\n", voxelizer.LastError()); return 1; }
	if (voxelizer.Thickness(DXV_COMP_SOLID, 1) || voxelizer.Thickness(2, capSq)) { fprintf(stderr, "a bad argument accepted\n"); return 1; }
	for (int of = DXV_COMP_EMPTY; of >= DXV_COMP_SOLID; --of) {
		float ms = 0.0f;
		uint64_t centres = 0, items = 0;
		if (!voxelizer.Thickness(of, capSq, of == DXV_COMP_SOLID) || !voxelizer.ThicknessField(field) || !voxelizer.ThicknessHistogram(histogram) ||
			!voxelizer.ThicknessInfo(ms, centres, items))
		{ fprintf(stderr, "Thickness: %s\n", voxelizer.LastError()); return 1; }
		if (field.size() != static_cast<size_t>(gridDim) * gridDim * gridDim || histogram.size() != capSq + 1u || !voxelizer.DeviceThickness()) return 1;
		uint32_t largest = 0, wall = 0;
		for (uint32_t v = 1; v <= capSq; ++v) {
			if (histogram[v] && !wall) wall = v;
			if (histogram[v]) largest = v;
		}
		printf("%llu %u %u %.3f %llu %llu\n", static_cast<unsigned long long>(field.size() - histogram[0]), largest, wall, Voxelizer::ThicknessVoxels(wall),
			static_cast<unsigned long long>(centres), static_cast<unsigned long long>(items));
	}
	FILE* f = fopen(argv[5], "wb");
	if (!f) return 1;
	fwrite(field.data(), sizeof(uint32_t), field.size(), f);
	fclose(f);
	return 0;
}
