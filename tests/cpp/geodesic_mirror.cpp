// The geodesic distance through the host-side C++ mirror include/dxv_voxelizer.hpp: InitFromArrays, Voxelize, Geodesic from the border and from a
// list of one voxel, the tally, the path from the farthest voxel.  Writes the map of the second run and its path; prints the two tallies.
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

static bool write_words(const char* path, const std::vector<uint32_t>& words)
{
	FILE* f = fopen(path, "wb");
	if (!f) return false;
	fwrite(words.data(), sizeof(uint32_t), words.size(), f);
	fclose(f);
	return true;
}

int main(int argc, char** argv)
{
	if (argc < 6) { fprintf(stderr, "usage: %s vb.bin ib.bin gridDim map.bin path.bin\n", argv[0]); return 2; }
	const std::vector<uint8_t> vb = read_file(argv[1]), ib = read_file(argv[2]);
	if (vb.empty() || ib.empty()) { fprintf(stderr, "cannot read the mesh\n"); return 1; }
	const uint32_t gridDim = static_cast<uint32_t>(atoi(argv[3]));
	Voxelizer voxelizer;
	if (!voxelizer.InitFromArrays(reinterpret_cast<const float*>(vb.data()), static_cast<uint32_t>(vb.size() / 24),
		reinterpret_cast<const uint32_t*>(ib.data()), static_cast<uint32_t>(ib.size() / 12)))
	{ fprintf(stderr, "Init failed: %s\n", voxelizer.LastError()); return 1; }
	std::vector<uint32_t> field, path;
	if (voxelizer.GeodesicField(field)) { fprintf(stderr, "a map before the first launch\n"); return 1; }
	if (!voxelizer.Voxelize(gridDim, Voxelizer::REFERENCE)) { fprintf(stderr, "Voxelize: %s\n", voxelizer.LastError()); return 1; }
	if (voxelizer.Geodesic(2, DXV_GEO_FACES) || voxelizer.Geodesic(DXV_COMP_SOLID, 2)) { fprintf(stderr, "a bad argument accepted\n"); return 1; }
	Voxelizer::GeodesicTally t;
	if (!voxelizer.Geodesic(DXV_COMP_EMPTY, DXV_GEO_FACES, 0, false) || !voxelizer.GeodesicField(field) || !voxelizer.GeodesicInfo(t))
	{ fprintf(stderr, "Geodesic: %s\n", voxelizer.LastError()); return 1; }
	printf("%llu %llu %llu %u %u\n", static_cast<unsigned long long>(t.seedsUsed), static_cast<unsigned long long>(t.reached), static_cast<unsigned long long>(t.unreached), t.farthest, t.farthestVoxel);
	uint32_t first = 0;
	while (first < field.size() && field[first] != DXV_GEO_NONE) ++first;      // the smallest solid voxel: no member of the empty space
	if (first == field.size()) { fprintf(stderr, "no solid voxel\n"); return 1; }
	if (!voxelizer.Geodesic(DXV_COMP_SOLID, DXV_GEO_CHAMFER, std::vector<uint32_t>{first}) || !voxelizer.GeodesicField(field) || !voxelizer.GeodesicInfo(t) ||
		!voxelizer.GeodesicPath(t.farthestVoxel, path))
	{ fprintf(stderr, "Geodesic: %s\n", voxelizer.LastError()); return 1; }
	if (field.size() != static_cast<size_t>(gridDim) * gridDim * gridDim || !voxelizer.DeviceGeodesic() || path.empty() || path.front() != t.farthestVoxel || path.back() != first) return 1;
	printf("%llu %llu %llu %u %u\n", static_cast<unsigned long long>(t.seedsUsed), static_cast<unsigned long long>(t.reached), static_cast<unsigned long long>(t.unreached), t.farthest, t.farthestVoxel);
	return write_words(argv[4], field) && write_words(argv[5], path) ? 0 : 1;
}
