// The skeleton graph through the host-side C++ mirror include/dxv_voxelizer.hpp: InitFromArrays, Voxelize(SURFACE), Fill, Thin to curves, then
// Skeleton (enqueued only, then read), a prune at the given bound, Thin and Skeleton again -- the header's recipe.  Writes the thinned grid, the
// labels, nodes and branches of the first skeleton and the grid after the prune; prints the first skeleton's counts, what the prune removed and
// the second skeleton's counts.
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

template <class T> static bool write_all(const char* path, const std::vector<T>& v)
{
	FILE* f = fopen(path, "wb");
	if (!f) return false;
	fwrite(v.data(), sizeof(T), v.size(), f);
	fclose(f);
	return true;
}

static void print(const Voxelizer::SkeletonCounts& c)
{
	printf("%u %u %llu %llu %llu\n", c.nodes, c.branches, static_cast<unsigned long long>(c.endVoxels), static_cast<unsigned long long>(c.curveVoxels),
		static_cast<unsigned long long>(c.junctionVoxels));
}

int main(int argc, char** argv)
{
	if (argc < 10) { fprintf(stderr, "usage: %s vb.bin ib.bin gridDim maxLen345 grid.bin labels.bin nodes.bin branches.bin pruned.bin\n", argv[0]); return 2; }
	const std::vector<uint8_t> vb = read_file(argv[1]), ib = read_file(argv[2]);
	if (vb.empty() || ib.empty()) { fprintf(stderr, "cannot read the mesh\n"); return 1; }
	const uint32_t gridDim = static_cast<uint32_t>(atoi(argv[3])), bound = static_cast<uint32_t>(atoi(argv[4]));
	Voxelizer voxelizer;
	if (!voxelizer.InitFromArrays(reinterpret_cast<const float*>(vb.data()), static_cast<uint32_t>(vb.size() / 24),
		reinterpret_cast<const uint32_t*>(ib.data()), static_cast<uint32_t>(ib.size() / 12)))
	{ fprintf(stderr, "Init failed: %s\n", voxelizer.LastError()); return 1; }
	std::vector<uint32_t> labels;
	std::vector<Voxelizer::SkeletonNode> nodes;
	std::vector<Voxelizer::SkeletonBranch> branches;
	std::vector<uint8_t> grid, pruned;
	if (voxelizer.SkeletonLabels(labels) || voxelizer.Skeleton()) { fprintf(stderr, "a skeleton before the first launch\n"); return 1; }
	if (!voxelizer.Voxelize(gridDim, Voxelizer::SURFACE) || !voxelizer.Fill() || !voxelizer.Thin(DXV_THIN_CURVE)) { fprintf(stderr, "Voxelize, Fill, Thin: %s\n", voxelizer.LastError()); return 1; }
	if (voxelizer.SkeletonPrune(bound)) { fprintf(stderr, "a prune without a skeleton\n"); return 1; }
	Voxelizer::SkeletonCounts c;
	if (!voxelizer.Skeleton(nullptr, false) || !voxelizer.SkeletonLabels(labels) || !voxelizer.SkeletonNodes(nodes) || !voxelizer.SkeletonBranches(branches) || !voxelizer.SkeletonInfo(c))
	{ fprintf(stderr, "Skeleton: %s\n", voxelizer.LastError()); return 1; }
	if (!voxelizer.DeviceSkeletonLabels() || c.nodes != nodes.size() || c.branches != branches.size() || !voxelizer.Download(grid)) return 1;
	print(c);
	uint32_t gone = 0;
	uint64_t voxels = 0;
	if (!voxelizer.SkeletonPrune(bound) || !voxelizer.SkeletonPruneInfo(gone, voxels) || !voxelizer.Download(pruned)) { fprintf(stderr, "SkeletonPrune: %s\n", voxelizer.LastError()); return 1; }
	printf("%u %llu\n", gone, static_cast<unsigned long long>(voxels));
	std::vector<Voxelizer::SkeletonNode> nodes2;
	if (voxelizer.SkeletonNodes(nodes2) || voxelizer.DeviceSkeletonLabels()) { fprintf(stderr, "a skeleton that is stale handed out\n"); return 1; }
	if (!voxelizer.Thin(DXV_THIN_CURVE) || !voxelizer.Skeleton() || !voxelizer.SkeletonInfo(c) || !voxelizer.SkeletonNodes(nodes2)) { fprintf(stderr, "Skeleton: %s\n", voxelizer.LastError()); return 1; }
	print(c);
	return write_all(argv[5], grid) && write_all(argv[6], labels) && write_all(argv[7], nodes) && write_all(argv[8], branches) && write_all(argv[9], pruned) ? 0 : 1;
}
