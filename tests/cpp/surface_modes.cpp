// The surface modes through the host-side C++ mirror include/dxv_voxelizer.hpp: InitFromArrays, then Voxelize(gridDim,
// Voxelizer::SURFACE) and Voxelize(gridDim, Voxelizer::REFERENCE_SURFACE).  Prints the two voxel counts; writes the surface grid.
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
	if (argc < 5) { fprintf(stderr, "usage: %s vb.bin ib.bin gridDim surface.bin\n", argv[0]); return 2; }
	const std::vector<uint8_t> vb = read_file(argv[1]), ib = read_file(argv[2]);
	if (vb.empty() || ib.empty()) { fprintf(stderr, "cannot read the mesh\n"); return 1; }
	const uint32_t gridDim = static_cast<uint32_t>(atoi(argv[3]));
	Voxelizer voxelizer;
	if (!voxelizer.InitFromArrays(reinterpret_cast<const float*>(vb.data()), static_cast<uint32_t>(vb.size() / 24),
		reinterpret_cast<const uint32_t*>(ib.data()), static_cast<uint32_t>(ib.size() / 12)))
	{ fprintf(stderr, "Init failed: %s\n", voxelizer.LastError()); return 1; }
	uint64_t surface = 0, shell = 0;
	std::vector<uint8_t> grid;
	if (!voxelizer.Voxelize(gridDim, Voxelizer::SURFACE) || !voxelizer.CountSolid(surface) || !voxelizer.Download(grid))
	{ fprintf(stderr, "surface: %s\n", voxelizer.LastError()); return 1; }
	if (!voxelizer.Voxelize(gridDim, Voxelizer::REFERENCE_SURFACE) || !voxelizer.CountSolid(shell))
	{ fprintf(stderr, "reference + surface: %s\n", voxelizer.LastError()); return 1; }
	if (voxelizer.Voxelize(gridDim, static_cast<Voxelizer::Mode>(4))) { fprintf(stderr, "mode 4 accepted\n"); return 1; }
	FILE* f = fopen(argv[4], "wb");
	if (!f) return 1;
	fwrite(grid.data(), 1, grid.size(), f);
	fclose(f);
	printf("%llu %llu\n", static_cast<unsigned long long>(surface), static_cast<unsigned long long>(shell));
	return 0;
}
