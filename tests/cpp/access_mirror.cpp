// The access radius and the intrusion map through the host-side C++ mirror include/dxv_voxelizer.hpp: InitFromArrays, Voxelize, Access of the
// empty space from the border with the intrusion map (enqueued only, then read), and of the solid from a list of one voxel without it.  Writes
// the two maps of the first run and the access map of the second; prints the two tallies.
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

static void print(const Voxelizer::AccessTally& t)
{
	printf("%llu %llu %llu %u %u\n", static_cast<unsigned long long>(t.seedsUsed), static_cast<unsigned long long>(t.reached), static_cast<unsigned long long>(t.unreached), t.widest, t.widestVoxel);
}

int main(int argc, char** argv)
{
	if (argc < 7) { fprintf(stderr, "usage: %s vb.bin ib.bin gridDim access.bin intrusion.bin access2.bin\n", argv[0]); return 2; }
	const std::vector<uint8_t> vb = read_file(argv[1]), ib = read_file(argv[2]);
	if (vb.empty() || ib.empty()) { fprintf(stderr, "cannot read the mesh\n"); return 1; }
	const uint32_t gridDim = static_cast<uint32_t>(atoi(argv[3]));
	Voxelizer voxelizer;
	if (!voxelizer.InitFromArrays(reinterpret_cast<const float*>(vb.data()), static_cast<uint32_t>(vb.size() / 24),
		reinterpret_cast<const uint32_t*>(ib.data()), static_cast<uint32_t>(ib.size() / 12)))
	{ fprintf(stderr, "Init failed: %s\n", voxelizer.LastError()); return 1; }
	std::vector<uint32_t> access, intrusion, second;
	std::vector<uint64_t> histA, histI;
	if (voxelizer.AccessField(access)) { fprintf(stderr, "a map before the first launch\n"); return 1; }
	if (!voxelizer.Voxelize(gridDim, Voxelizer::REFERENCE)) { fprintf(stderr, "Voxelize: %s\n", voxelizer.LastError()); return 1; }
	if (voxelizer.Access(2) || voxelizer.Access(DXV_COMP_EMPTY, 18) || voxelizer.Access(DXV_COMP_EMPTY, 26, 1)) { fprintf(stderr, "a bad argument accepted\n"); return 1; }
	Voxelizer::AccessTally t;
	if (!voxelizer.Access(DXV_COMP_EMPTY, 6, 65, true, false) || !voxelizer.AccessField(access) || !voxelizer.IntrusionField(intrusion) || !voxelizer.AccessHistogram(histA) ||
		!voxelizer.IntrusionHistogram(histI) || !voxelizer.AccessInfo(t))
	{ fprintf(stderr, "Access: %s\n", voxelizer.LastError()); return 1; }
	if (histA.size() != 66 || histI.size() != 66 || !voxelizer.DeviceAccess() || !voxelizer.DeviceIntrusion()) return 1;
	print(t);
	std::vector<uint8_t> grid;
	if (!voxelizer.Download(grid)) { fprintf(stderr, "Download: %s\n", voxelizer.LastError()); return 1; }
	uint32_t first = 0;
	while (first < grid.size() && !grid[first]) ++first;               // the smallest solid voxel
	if (first == grid.size()) { fprintf(stderr, "no solid voxel\n"); return 1; }
	if (!voxelizer.Access(DXV_COMP_SOLID, 26, 4096, std::vector<uint32_t>{first, first}, false) || !voxelizer.AccessField(second) || !voxelizer.AccessInfo(t))
	{ fprintf(stderr, "Access: %s\n", voxelizer.LastError()); return 1; }
	if (voxelizer.IntrusionField(intrusion) || voxelizer.DeviceIntrusion()) { fprintf(stderr, "an intrusion map that was not asked for\n"); return 1; }
	if (second.size() != static_cast<size_t>(gridDim) * gridDim * gridDim) return 1;
	print(t);
	if (!voxelizer.Access(DXV_COMP_EMPTY, 6, 65) || !voxelizer.IntrusionField(intrusion)) { fprintf(stderr, "Access: %s\n", voxelizer.LastError()); return 1; }
	return write_words(argv[4], access) && write_words(argv[5], intrusion) && write_words(argv[6], second) ? 0 : 1;
}
