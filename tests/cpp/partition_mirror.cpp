// The maximal-ball partition through the host-side C++ mirror include/dxv_voxelizer.hpp: InitFromArrays, Voxelize, Partition for both kinds, then
// labels, table and throats.  Writes the solid labels; prints, per kind, the members, K, T, the interface faces, the largest region's voxels and
// radius^2 and the widest neck.
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
	if (argc < 6) { fprintf(stderr, "usage: %s vb.bin ib.bin gridDim capSq labels.bin\n", argv[0]); return 2; }
	const std::vector<uint8_t> vb = read_file(argv[1]), ib = read_file(argv[2]);
	if (vb.empty() || ib.empty()) { fprintf(stderr, "cannot read the mesh\n"); return 1; }
	const uint32_t gridDim = static_cast<uint32_t>(atoi(argv[3])), capSq = static_cast<uint32_t>(atoi(argv[4]));
	Voxelizer voxelizer;
	if (!voxelizer.InitFromArrays(reinterpret_cast<const float*>(vb.data()), static_cast<uint32_t>(vb.size() / 24),
		reinterpret_cast<const uint32_t*>(ib.data()), static_cast<uint32_t>(ib.size() / 12)))
	{ fprintf(stderr, "Init failed: %s\n", voxelizer.LastError()); return 1; }
	std::vector<uint32_t> labels;
	std::vector<Voxelizer::PartitionRegion> table;
	std::vector<Voxelizer::PartitionThroat> throats;
	if (voxelizer.PartitionLabels(labels) || voxelizer.PartitionTable(table)) { fprintf(stderr, "a partition before the first launch\n"); return 1; }
	if (!voxelizer.Voxelize(gridDim, Voxelizer::REFERENCE)) { fprintf(stderr, "Voxelize: %s\n", voxelizer.LastError()); return 1; }
	if (voxelizer.Partition(DXV_COMP_SOLID, 0) || voxelizer.Partition(2, capSq)) { fprintf(stderr, "a bad argument accepted\n"); return 1; }
	if (!voxelizer.Partition(DXV_COMP_SOLID, capSq, false) || voxelizer.PartitionThroats(throats)) { fprintf(stderr, "throats of a partition made without them\n"); return 1; }
	for (int of = DXV_COMP_EMPTY; of >= DXV_COMP_SOLID; --of) {
		float ms = 0.0f;
		uint32_t regions = 0, count = 0;
		uint64_t faces = 0;
		if (!voxelizer.Partition(of, capSq, true, of == DXV_COMP_SOLID) || !voxelizer.PartitionLabels(labels) || !voxelizer.PartitionTable(table) ||
			!voxelizer.PartitionThroats(throats) || !voxelizer.PartitionInfo(ms, regions, count, faces))
		{ fprintf(stderr, "Partition: %s\n", voxelizer.LastError()); return 1; }
		if (labels.size() != static_cast<size_t>(gridDim) * gridDim * gridDim || table.size() != regions || throats.size() != count || !voxelizer.DevicePartitionLabels()) return 1;
		uint64_t members = 0;
		for (uint32_t l : labels) members += l != 0u;
		uint32_t largest = 0, radius = 0, neck = 0;
		for (const Voxelizer::PartitionRegion& r : table)
			if (r.voxels > largest) { largest = r.voxels; radius = r.radiusSq; }
		for (const Voxelizer::PartitionThroat& t : throats)
			if (t.neckSq > neck) neck = t.neckSq;
		printf("%llu %u %u %llu %u %u %u\n", static_cast<unsigned long long>(members), regions, count, static_cast<unsigned long long>(faces), largest, radius, neck);
	}
	FILE* f = fopen(argv[5], "wb");
	if (!f) return 1;
	fwrite(labels.data(), sizeof(uint32_t), labels.size(), f);
	fclose(f);
	return 0;
}
