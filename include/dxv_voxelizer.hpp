// dxv_voxelizer.hpp -- host-side C++ mirror of the reference's Voxelizer component over the
// C-ABI (include/dxv.h).  Header only; link with libdxv.so.
//
// Reference surface (Content/Voxelizer.h:10-24):
//   bool Init(pCommandList, descriptorTableLib, width, height, rtFormat, dsFormat, uploaders,
//             pGeometry, fileName, posScale);
//   void UpdateFrame(frameIndex, eyePt, viewProj);  void Render(pCommandList, frameIndex, rtv, dsv);
//   protected: void voxelize(pCommandList, frameIndex);   // the hot call, GRID_SIZE = 64 macro
//
// Here: the D3D12-only parameters are gone (command lists, descriptor tables, formats, uploaders; the render target is a
// device pointer and its row pitch, the viewport is SetViewport's); `voxelize` is public as Voxelize(gridDim) with the
// grid size promoted from the GRID_SIZE macro (Content/Voxelizer.cpp:8) to a parameter; every
// fallible call returns bool like the reference (XUSG/Core/XUSG.h:12-15) and never throws.
// posScale is accepted and, exactly as in the reference, does not affect voxelisation
// (Content/Voxelizer.cpp:84-87 uses it for display matrices only).
#pragma once
#include "dxv.h"

#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

class Voxelizer
{
public:
	enum Mode : int { REFERENCE = DXV_MODE_REFERENCE, PARITY = DXV_MODE_PARITY, SURFACE = DXV_MODE_SURFACE, REFERENCE_SURFACE = DXV_MODE_REFERENCE_SURFACE };

	explicit Voxelizer(int device = 0) : m_device(device) {}
	virtual ~Voxelizer() { dxv_destroy(m_ctx); }
	Voxelizer(const Voxelizer&) = delete;
	Voxelizer& operator=(const Voxelizer&) = delete;

	// Load the OBJ, upload VB/IB, extract the bound, build the acceleration structure
	// (Content/Voxelizer.cpp:30-79).  Like the reference's Init (:73: buildAccelerationStructures), it leaves EVERYTHING the
	// launches trace through finished -- the LBVH and the candidate lists of the reference rule on the map a static scene is
	// launched with: the first Voxelize costs what every later one costs.
	// gridDim: the grid the scene will be voxelized at -- the reference's GRID_SIZE, which is a compile-time constant there
	// (Content/Voxelizer.cpp:8) and so is known to its Init as well.  The scene's work queue for that grid is then built here too
	// (dxv_prepare_launch) and every Voxelize(gridDim) is one dispatch behind a clear (Content/Voxelizer.cpp:351-369); 0: launches build
	// their queue themselves.
	bool Init(const char* fileName, const float posScale[4] = nullptr, bool dynamicMesh = false, uint32_t gridDim = 0)
	{
		float* vb = nullptr; uint32_t* ib = nullptr; uint32_t numVerts = 0, numIndices = 0; float aabb[6];
		if (dxv_obj_load(fileName, &vb, &numVerts, &ib, &numIndices, aabb)) return setError("cannot load OBJ file");
		const bool ok = InitFromArrays(vb, numVerts, ib, numIndices / 3, posScale, dynamicMesh, gridDim);
		dxv_free(vb); dxv_free(ib);
		return ok;
	}

	// Same from memory: vb = numVerts x {pos.xyz, nrm.xyz}, ib = 3*numTris indices, both in the
	// layout ObjLoader produces (createVB/createIB, Content/Voxelizer.cpp:115-138).
	// dynamicMesh: the vertices will be replaced and the hierarchy refitted every frame (UpdateVertices*): only the LBVH is
	// built here, and every frame's lists are built for that frame on the coarser map (include/dxv.h, option lists).
	bool InitFromArrays(const float* vb, uint32_t numVerts, const uint32_t* ib, uint32_t numTris,
		const float posScale[4] = nullptr, bool dynamicMesh = false, uint32_t gridDim = 0)
	{
		for (int i = 0; i < 4; ++i) m_posScale[i] = posScale ? posScale[i] : (i == 3 ? 1.0f : 0.0f);
		if (!m_ctx && dxv_create(&m_ctx, m_device)) return setError(dxv_last_error(nullptr));
		if (dxv_set_mesh(m_ctx, vb, numVerts, ib, numTris)) return false;
		if (dxv_build(m_ctx)) return false;
		return dynamicMesh || dxv_build_lists_for_grid(m_ctx, gridDim) == 0;
	}
	// the work queue of another grid size or of a slab, built now (dxv_prepare_launch)
	bool PrepareLaunch(uint32_t gridDim) { return PrepareLaunch(gridDim, 0, gridDim); }
	bool PrepareLaunch(uint32_t gridDim, uint32_t z0, uint32_t nz)
	{
		if (!m_ctx) return setError("PrepareLaunch before Init");
		return dxv_prepare_launch(m_ctx, gridDim, z0, nz) == 0;
	}
	bool InitDynamic(const float* vb, uint32_t numVerts, const uint32_t* ib, uint32_t numTris, const float posScale[4] = nullptr)
	{
		return InitFromArrays(vb, numVerts, ib, numTris, posScale, true);
	}

	// The hot call (Content/Voxelizer.cpp:351-369): whole grid, or slices [z0, z0+nz).
	bool Voxelize(uint32_t gridDim, Mode mode = REFERENCE) { return Voxelize(gridDim, mode, 0, gridDim); }
	bool Voxelize(uint32_t gridDim, Mode mode, uint32_t z0, uint32_t nz)
	{
		if (!m_ctx) return setError("Voxelize before Init");
		return dxv_voxelize(m_ctx, gridDim, mode, z0, nz) == 0;
	}

	// Frames in flight, as the reference's per-frame calls take a frameIndex (Content/Voxelizer.h:20-22) and the
	// component owns FrameCount grids (:24, :110): VoxelizeAsync(frameIndex, ...) launches into that frame's grid on
	// that frame's stream and returns; WaitFrame(frameIndex) waits for it and reports a deferred kernel error.
	// Download / DownloadBits / CountSolid / DeviceGrid / Render then refer to the frame last selected.
	bool SetFrame(uint8_t frameIndex) { return m_ctx ? dxv_set_frame(m_ctx, frameIndex) == 0 : setError("SetFrame before Init"); }
	bool VoxelizeAsync(uint8_t frameIndex, uint32_t gridDim, Mode mode = REFERENCE)
	{
		return SetFrame(frameIndex) && dxv_voxelize_async(m_ctx, gridDim, mode, 0, gridDim) == 0;
	}
	bool WaitFrame(uint8_t frameIndex) { return SetFrame(frameIndex) && dxv_sync(m_ctx) == 0; }
	bool WaitAll() { return m_ctx && dxv_sync_all(m_ctx) == 0; }

	// Dynamic meshes: new vertex data on the same topology, refit of the existing hierarchy.
	bool UpdateVertices(const float* vb, uint32_t numVerts)
	{
		if (!m_ctx) return setError("UpdateVertices before Init");
		return dxv_update_vertices(m_ctx, vb, numVerts) == 0 && dxv_refit(m_ctx) == 0;
	}

	// The two halves on their own, for a loop that hides the upload: VoxelizeAsync(frame i); UploadVertices(frame i + 1) --
	// dxv_update_vertices does not wait for launches in flight, they read the scene and not the vertex buffer --;
	// Refit() (the frame's one host round trip: its kernels and the lists' counting pass queue up behind the launch);
	// VoxelizeAsync(frame i + 1) (queued behind the list build); ...  From a pose already on the GPU: UpdateVerticesDevice.
	bool UploadVertices(const float* vb, uint32_t numVerts)
	{
		if (!m_ctx) return setError("UploadVertices before Init");
		return dxv_update_vertices(m_ctx, vb, numVerts) == 0;
	}
	bool Refit() { return m_ctx ? dxv_refit(m_ctx) == 0 : setError("Refit before Init"); }

	// ... from a device buffer (a mesh animated on the GPU)
	bool UpdateVerticesDevice(const void* deviceVb, uint32_t numVerts)
	{
		if (!m_ctx) return setError("UpdateVerticesDevice before Init");
		return dxv_update_vertices_device(m_ctx, deviceVb, numVerts) == 0 && dxv_refit(m_ctx) == 0;
	}

	// Content/Voxelizer.h:20-22: UpdateFrame(frameIndex, eyePt, viewProj) stores the camera, Render
	// runs voxelize + the ray-cast display pass.  eyePt[3]; viewProj row-major, row vectors
	// (XMFLOAT4X4 of view * proj, DXRVoxelizer.cpp:249-254).
	void UpdateFrame(const float eyePt[3], const float viewProj[16])
	{
		for (int i = 0; i < 3; ++i) m_eyePt[i] = eyePt[i];
		for (int i = 0; i < 16; ++i) m_viewProj[i] = viewProj[i];
	}
	bool Render(uint32_t gridDim, uint32_t width, uint32_t height, std::vector<uint8_t>& rgba)
	{
		if (!Voxelize(gridDim)) return false;
		rgba.resize(static_cast<size_t>(width) * height * 4);
		return dxv_render(m_ctx, m_eyePt, m_viewProj, m_posScale, width, height, rgba.data()) == 0;
	}

	// The reference's frame loop (Content/Voxelizer.cpp:81-113, :371-399): FrameCount frames in flight, each with its own
	// constants and its own render target on the GPU, and no host wait for an image.
	//   SetViewport(width, height)                     the width / height the reference's Init receives (default 1280 x 720)
	//   UpdateFrame(frameIndex, eyePt, viewProj)        that frame's ray-cast constants (dxv_update_frame)
	//   Render(frameIndex, gridDim, deviceRgba, pitch)  VoxelizeAsync + the ray-cast into width x height R8G8B8A8 texels at
	//                                                  deviceRgba (device memory, rows pitch bytes apart), enqueued (dxv_render_async)
	//   WaitFrameOn(frameIndex, hipStream)             a consumer's stream waits on the device for that frame (dxv_stream_wait_frame)
	// WaitFrame / WaitAll report the launches' and renders' errors.  Ordering the render targets is the caller's, as in the
	// reference (one render target per frame).
	void SetViewport(uint32_t width, uint32_t height) { m_width = width; m_height = height; }
	bool UpdateFrame(uint8_t frameIndex, const float eyePt[3], const float viewProj[16])
	{
		if (!SetFrame(frameIndex)) return false;
		return dxv_update_frame(m_ctx, eyePt, viewProj, m_posScale, m_width, m_height) == 0;
	}
	bool Render(uint8_t frameIndex, uint32_t gridDim, void* deviceRgba, size_t rowPitch)
	{
		return VoxelizeAsync(frameIndex, gridDim) && dxv_render_async(m_ctx, deviceRgba, rowPitch) == 0;
	}
	bool WaitFrameOn(uint8_t frameIndex, void* hipStream) { return SetFrame(frameIndex) && dxv_stream_wait_frame(m_ctx, hipStream) == 0; }

	// The exact signed distance field of that frame's whole grid (dxv_distance_async: enqueued behind the frame's launch, 4 bytes per
	// voxel, DXV_DIST_SQ_I32 or DXV_DIST_F32, negative inside, voxel units centre to centre).  DeviceDistance / DownloadDistance refer to
	// the frame last selected; WaitFrame reports the kernels' errors.
	bool DistanceField(uint8_t frameIndex, int format = DXV_DIST_F32) { return SetFrame(frameIndex) && dxv_distance_async(m_ctx, format) == 0; }
	const void* DeviceDistance() const { return m_ctx ? dxv_distance_device_ptr(m_ctx) : nullptr; }
	bool DownloadDistance(std::vector<uint8_t>& field)
	{
		if (!m_ctx) return setError("DownloadDistance before Init");
		field.resize(dxv_distance_bytes(m_ctx));
		return dxv_distance_download(m_ctx, field.data(), field.size()) == 0;
	}

	// The exact distance from the voxel centres of that frame's last launch to the mesh, signed by the frame's grid (dxv_mesh_distance_async:
	// enqueued behind the frame's launch and fill, one float per voxel, DXV_MDIST_VOXELS_F32 or DXV_MDIST_UNITS_F32; bandVoxels > 0 caps it).
	// DeviceMeshDistance / DownloadMeshDistance refer to the frame last selected; WaitFrame reports the kernel's errors.
	bool MeshDistanceField(uint8_t frameIndex, int format = DXV_MDIST_VOXELS_F32, uint32_t bandVoxels = 0, bool triangles = false)
	{
		return SetFrame(frameIndex) && dxv_mesh_distance_async(m_ctx, format, bandVoxels, triangles ? 1 : 0) == 0;
	}
	const void* DeviceMeshDistance() const { return m_ctx ? dxv_mesh_distance_device_ptr(m_ctx) : nullptr; }
	bool DownloadMeshDistance(std::vector<float>& field)
	{
		if (!m_ctx) return setError("DownloadMeshDistance before Init");
		field.resize(dxv_mesh_distance_bytes(m_ctx) / sizeof(float));
		return dxv_mesh_distance_download(m_ctx, field.data(), field.size() * sizeof(float)) == 0;
	}

	// The isosurface of one of that frame's fields as a closed triangle mesh (dxv_isosurface_async: naive Surface Nets on the device; source
	// DXV_ISO_MESH_DISTANCE or DXV_ISO_GRID_DISTANCE, the mesh in DXV_ISO_SPACE_OBJECT -- the space of the mesh Init was given -- or in
	// DXV_ISO_SPACE_VOXELS).  The buffers have the layout Init's own take: 6 floats per vertex, 3 uint32 per triangle.  IsosurfaceCounts,
	// DeviceIsosurface* and DownloadIsosurface refer to the frame last selected; WaitFrame reports the kernels' errors.
	bool Isosurface(uint8_t frameIndex, int source = DXV_ISO_MESH_DISTANCE, float iso = 0.0f, int space = DXV_ISO_SPACE_OBJECT)
	{
		return SetFrame(frameIndex) && dxv_isosurface_async(m_ctx, source, iso, space) == 0;
	}
	bool IsosurfaceCounts(uint32_t& vertices, uint32_t& triangles) { return m_ctx && dxv_isosurface_counts(m_ctx, &vertices, &triangles) == 0; }
	const void* DeviceIsosurfaceVertices() const { return m_ctx ? dxv_isosurface_vertices_device_ptr(m_ctx) : nullptr; }
	const void* DeviceIsosurfaceIndices() const { return m_ctx ? dxv_isosurface_indices_device_ptr(m_ctx) : nullptr; }
	bool DownloadIsosurface(std::vector<float>& vb, std::vector<uint32_t>& ib)
	{
		uint32_t vertices = 0, triangles = 0;
		if (!m_ctx) return setError("DownloadIsosurface before Init");
		if (dxv_isosurface_counts(m_ctx, &vertices, &triangles)) return false;
		vb.resize(6 * (size_t)vertices);
		ib.resize(3 * (size_t)triangles);
		return dxv_isosurface_vertices_download(m_ctx, vb.data(), vb.size() * sizeof(float)) == 0 &&
		       dxv_isosurface_indices_download(m_ctx, ib.data(), ib.size() * sizeof(uint32_t)) == 0;
	}
	bool IsosurfaceMs(float& ms) { return m_ctx && dxv_isosurface_ms(m_ctx, &ms) == 0; }

	// The sparse voxel octree of that frame's grid (dxv_octree_async: one 8-byte node for the root and for every mixed cell; include/dxv.h has
	// the rule), enqueued behind the frame's launch.  OctreeInfo, DeviceOctree and DownloadOctree refer to the frame last selected;
	// WaitFrame reports the kernels' errors.  OctreeExpand writes the frame's grid from a tree on this device (nullptr: the frame's own).
	bool Octree(uint8_t frameIndex) { return SetFrame(frameIndex) && dxv_octree_async(m_ctx) == 0; }
	bool OctreeInfo(uint32_t& levels, uint32_t& nodes, uint32_t levelFirst[12]) { return m_ctx && dxv_octree_info(m_ctx, &levels, &nodes, levelFirst) == 0; }
	const void* DeviceOctree() const { return m_ctx ? dxv_octree_device_ptr(m_ctx) : nullptr; }
	bool DownloadOctree(std::vector<uint32_t>& nodes)
	{
		if (!m_ctx) return setError("DownloadOctree before Init");
		nodes.resize(dxv_octree_bytes(m_ctx) / sizeof(uint32_t));
		return dxv_octree_download(m_ctx, nodes.data(), nodes.size() * sizeof(uint32_t)) == 0;
	}
	bool OctreeMs(float& ms) { return m_ctx && dxv_octree_ms(m_ctx, &ms) == 0; }
	bool OctreeExpand(uint8_t frameIndex, const void* deviceNodes = nullptr, uint32_t nodes = 0, uint32_t levels = 0)
	{
		return SetFrame(frameIndex) && dxv_octree_expand_async(m_ctx, deviceNodes, nodes, levels) == 0;
	}

	// The connected components of that frame's whole grid (dxv_components_async: labels 1 .. K by ascending smallest index and a 24-byte record per
	// component; include/dxv.h has the rule), enqueued behind the frame's launch.  The accessors refer to the frame last selected; WaitFrame
	// reports the kernels' errors.  SelectComponents edits the frame's grid in place from its labels: Components(f) && SelectComponents(
	// DXV_SELECT_LARGEST) removes floaters, Components(f, DXV_COMP_EMPTY) && SelectComponents(DXV_SELECT_MIN_VOXELS, m) closes cavities below m voxels.
	struct ComponentRecord { uint32_t first, voxels; uint16_t lo[3], hi[3]; uint32_t flags; };
	bool Components(uint8_t frameIndex, int of = DXV_COMP_SOLID, int connectivity = 6) { return SetFrame(frameIndex) && dxv_components_async(m_ctx, of, connectivity) == 0; }
	bool ComponentsInfo(uint32_t& count, int& of, int& connectivity) { return m_ctx && dxv_components_info(m_ctx, &count, &of, &connectivity) == 0; }
	const void* DeviceComponentLabels() const { return m_ctx ? dxv_components_labels_device_ptr(m_ctx) : nullptr; }
	const void* DeviceComponentTable() const { return m_ctx ? dxv_components_table_device_ptr(m_ctx) : nullptr; }
	bool DownloadComponents(std::vector<uint32_t>& labels, std::vector<ComponentRecord>& table)
	{
		if (!m_ctx) return setError("DownloadComponents before Init");
		static_assert(sizeof(ComponentRecord) == 24, "a row of the table is 24 bytes");
		labels.resize(dxv_components_labels_bytes(m_ctx) / sizeof(uint32_t));
		table.resize(dxv_components_table_bytes(m_ctx) / sizeof(ComponentRecord));
		return dxv_components_labels_download(m_ctx, labels.data(), labels.size() * sizeof(uint32_t)) == 0 &&
			dxv_components_table_download(m_ctx, table.data(), table.size() * sizeof(ComponentRecord)) == 0;
	}
	bool ComponentsMs(float& ms) { return m_ctx && dxv_components_ms(m_ctx, &ms) == 0; }
	bool SelectComponents(int rule, uint32_t arg = 0, bool sync = true)
	{
		return m_ctx && (sync ? dxv_components_select(m_ctx, rule, arg) : dxv_components_select_async(m_ctx, rule, arg)) == 0;
	}
	bool SelectInfo(uint32_t& kept, uint32_t& dropped, uint64_t& voxelsChanged) { return m_ctx && dxv_components_select_info(m_ctx, &kept, &dropped, &voxelsChanged) == 0; }

	// The integral measures of the selected frame's current labelling (dxv_measure / dxv_measure_async; include/dxv.h has the rule): a 96-byte
	// record per component and record 0 for all of them together.  MassProperties turns a record into volume, centroid (at voxel centres),
	// area and the inertia tensor about the centroid, in voxel units at unit density; the central second moments are formed exactly in 128 bits
	// before the one division.  Betti gives the pieces, handles and cavities of the solid as a complex of closed unit cubes: it labels the empty
	// space (6), then the solid (26), measures it, and leaves that labelling and its measure current.
	struct MeasureRecord { uint64_t voxels, sum[3], sum2[3], prod[3], faces; int64_t euler; };
	struct MassRecord { double volume, centroid[3], area, inertia[3][3]; };
	bool Measure(bool sync = true) { return m_ctx && (sync ? dxv_measure(m_ctx) : dxv_measure_async(m_ctx)) == 0; }
	const void* DeviceMeasureTable() const { return m_ctx ? dxv_measure_table_device_ptr(m_ctx) : nullptr; }
	bool MeasureTable(std::vector<MeasureRecord>& table)
	{
		if (!m_ctx) return setError("MeasureTable before Init");
		static_assert(sizeof(MeasureRecord) == 96, "a row of the table is 96 bytes");
		const size_t bytes = dxv_measure_table_bytes(m_ctx);
		if (!bytes) return false;
		table.resize(bytes / sizeof(MeasureRecord));
		return dxv_measure_table_download(m_ctx, table.data(), bytes) == 0;
	}
	bool MeasureMs(float& ms) { return m_ctx && dxv_measure_ms(m_ctx, &ms) == 0; }
	static MassRecord MassProperties(const MeasureRecord& r)
	{
		typedef unsigned __int128 u128;
		MassRecord out = {};
		out.volume = (double)r.voxels;
		out.area = (double)r.faces;
		if (!r.voxels) return out;
		const u128 V = r.voxels;
		u128 central[3];                                                   // V * the sum of (x - mean)^2 >= 0, exact
		for (int a = 0; a < 3; ++a) {
			central[a] = V * r.sum2[a] - (u128)r.sum[a] * r.sum[a];
			out.centroid[a] = (double)(2 * (u128)r.sum[a] + V) / (double)(2 * V);
		}
		for (int a = 0; a < 3; ++a) {
			const int b = (a + 1) % 3, c = (a + 2) % 3;
			out.inertia[a][a] = (double)(6 * (central[b] + central[c]) + V * V) / (double)(6 * V);
			const u128 pos = V * r.prod[a], neg = (u128)r.sum[a] * r.sum[b];   // prod[a] pairs axis a with axis a + 1: xy, yz, zx
			out.inertia[a][b] = out.inertia[b][a] = pos >= neg ? -((double)(pos - neg) / (double)V) : (double)(neg - pos) / (double)V;
		}
		return out;
	}
	bool Betti(uint32_t& b0, uint32_t& b1, uint32_t& b2)
	{
		if (!m_ctx) return setError("Betti before Init");
		if (dxv_components(m_ctx, DXV_COMP_EMPTY, 6)) return false;
		std::vector<ComponentRecord> empty(dxv_components_table_bytes(m_ctx) / sizeof(ComponentRecord));
		std::vector<MeasureRecord> table;
		if (dxv_components_table_download(m_ctx, empty.data(), empty.size() * sizeof(ComponentRecord))) return false;
		uint32_t cavities = 0, pieces = 0;
		for (const ComponentRecord& r : empty) cavities += (r.flags & 1u) ? 0u : 1u;
		int of = 0, connectivity = 0;
		if (dxv_components(m_ctx, DXV_COMP_SOLID, 26) || !ComponentsInfo(pieces, of, connectivity) || !Measure() || !MeasureTable(table)) return false;
		b0 = pieces; b2 = cavities;
		b1 = (uint32_t)((int64_t)pieces + (int64_t)cavities - table[0].euler);
		return true;
	}

	// The exact local thickness of the selected frame's whole grid (dxv_thickness / dxv_thickness_async; include/dxv.h has the rule): per member
	// voxel the squared radius of the largest voxel-centred ball inside the members that holds it, capped at capSq (2 .. 4096); of = DXV_COMP_EMPTY
	// measures channels and pores.  The grid and the frame's other products stay as they are.  ThicknessVoxels turns a squared radius into
	// voxels, 2 sqrt(W) - 1: a slab k voxels thick reads 2 ceil(k / 2) - 1, so even thicknesses read as the next odd one.
	bool Thickness(int of = DXV_COMP_SOLID, uint32_t capSq = 4096, bool sync = true) { return m_ctx && (sync ? dxv_thickness(m_ctx, of, capSq) : dxv_thickness_async(m_ctx, of, capSq)) == 0; }
	const void* DeviceThickness() const { return m_ctx ? dxv_thickness_device_ptr(m_ctx) : nullptr; }
	bool ThicknessField(std::vector<uint32_t>& field)
	{
		if (!m_ctx) return setError("ThicknessField before Init");
		const size_t bytes = dxv_thickness_bytes(m_ctx);
		if (!bytes) return false;
		field.resize(bytes / sizeof(uint32_t));
		return dxv_thickness_download(m_ctx, field.data(), bytes) == 0;
	}
	bool ThicknessHistogram(std::vector<uint64_t>& histogram)
	{
		if (!m_ctx) return setError("ThicknessHistogram before Init");
		const size_t bytes = dxv_thickness_histogram_bytes(m_ctx);
		if (!bytes) return false;
		histogram.resize(bytes / sizeof(uint64_t));
		return dxv_thickness_histogram_download(m_ctx, histogram.data(), bytes) == 0;
	}
	bool ThicknessInfo(float& ms, uint64_t& centresPainted, uint64_t& workItems) { return m_ctx && dxv_thickness_info(m_ctx, &ms, &centresPainted, &workItems) == 0; }
	static float ThicknessVoxels(uint32_t w) { return w ? 2.0f * sqrtf((float)w) - 1.0f : 0.0f; }

	// The maximal-ball partition of the selected frame's whole grid (dxv_partition / dxv_partition_async; include/dxv.h has the rule and the two
	// record layouts): regions -- pore bodies of the empty space, lobes of the solid -- as labels and a table of 32-byte records, and the throats
	// between them as 20-byte records.  The grid and the frame's other products stay as they are.  A region is a family of balls and need not be
	// 6-connected; choose capSq at least the largest radius^2 of interest; a tube of constant width is cut into pieces about its diameter long.
	struct PartitionRegion { uint32_t root, radiusSq, voxels, throats; uint16_t lo[3], hi[3]; uint32_t flags; };
	struct PartitionThroat { uint32_t a, b, faces, neckSq, neckVoxel; };
	bool Partition(int of = DXV_COMP_SOLID, uint32_t capSq = 4096, bool throats = true, bool sync = true)
	{
		return m_ctx && (sync ? dxv_partition(m_ctx, of, capSq, throats ? 1 : 0) : dxv_partition_async(m_ctx, of, capSq, throats ? 1 : 0)) == 0;
	}
	const void* DevicePartitionLabels() const { return m_ctx ? dxv_partition_labels_device_ptr(m_ctx) : nullptr; }
	bool PartitionLabels(std::vector<uint32_t>& labels)
	{
		if (!m_ctx) return setError("PartitionLabels before Init");
		const size_t bytes = dxv_partition_labels_bytes(m_ctx);
		if (!bytes) return dxv_partition_labels_device_ptr(m_ctx) != nullptr;      // (false, with the message: none yet, or stale)
		labels.resize(bytes / sizeof(uint32_t));
		return dxv_partition_labels_download(m_ctx, labels.data(), bytes) == 0;
	}
	bool PartitionTable(std::vector<PartitionRegion>& table)
	{
		if (!m_ctx) return setError("PartitionTable before Init");
		static_assert(sizeof(PartitionRegion) == 32, "a region record is 32 bytes");
		const size_t bytes = dxv_partition_table_bytes(m_ctx);
		table.resize(bytes / sizeof(PartitionRegion));
		return dxv_partition_table_download(m_ctx, table.data(), bytes) == 0;
	}
	bool PartitionThroats(std::vector<PartitionThroat>& throats)
	{
		if (!m_ctx) return setError("PartitionThroats before Init");
		static_assert(sizeof(PartitionThroat) == 20, "a throat record is 20 bytes");
		const size_t bytes = dxv_partition_throats_bytes(m_ctx);
		throats.resize(bytes / sizeof(PartitionThroat));
		return dxv_partition_throats_download(m_ctx, throats.data(), bytes) == 0;
	}
	bool PartitionInfo(float& ms, uint32_t& regions, uint32_t& throats, uint64_t& interfaceFaces) { return m_ctx && dxv_partition_info(m_ctx, &ms, &regions, &throats, &interfaceFaces) == 0; }

	// The skeleton graph of the selected frame's whole grid (dxv_skeleton / dxv_skeleton_async; include/dxv.h has the rule and the two record
	// layouts): a label per voxel -- 0, k for node k, 0x80000000 | b for branch b --, the nodes as 32-byte records and the branches as 48-byte
	// records.  deviceWeights: nullptr, or N^3 uint32 on the device laid out like the grid (another frame's DeviceThickness()): their minimum,
	// maximum and sum along every branch.  A graph of the shape for a grid Thin has left; a solid blob is one big node.  The grid and the frame's
	// other products stay as they are.  SkeletonPrune removes from the grid, in place, every spur with 3 steps[0] + 4 steps[1] + 5 steps[2] <=
	// maxLen345, with its tip; the recipe is Thin; Skeleton; SkeletonPrune(L); Thin; Skeleton.
	struct SkeletonNode { uint32_t first, voxels, degree, flags; uint16_t lo[3], hi[3]; uint32_t wMax; };
	struct SkeletonBranch { uint32_t a, b, first, voxels, steps[3], flags, wMin, wMax; uint64_t wSum; };
	struct SkeletonCounts { float ms; uint32_t nodes, branches; uint64_t endVoxels, curveVoxels, junctionVoxels; };
	bool Skeleton(const void* deviceWeights = nullptr, bool sync = true)
	{
		return m_ctx && (sync ? dxv_skeleton(m_ctx, deviceWeights) : dxv_skeleton_async(m_ctx, deviceWeights)) == 0;
	}
	const void* DeviceSkeletonLabels() const { return m_ctx ? dxv_skeleton_labels_device_ptr(m_ctx) : nullptr; }
	bool SkeletonLabels(std::vector<uint32_t>& labels)
	{
		if (!m_ctx) return setError("SkeletonLabels before Init");
		const size_t bytes = dxv_skeleton_labels_bytes(m_ctx);
		if (!bytes) return dxv_skeleton_labels_device_ptr(m_ctx) != nullptr;       // (false, with the message: none yet, or stale)
		labels.resize(bytes / sizeof(uint32_t));
		return dxv_skeleton_labels_download(m_ctx, labels.data(), bytes) == 0;
	}
	bool SkeletonNodes(std::vector<SkeletonNode>& nodes)
	{
		if (!m_ctx) return setError("SkeletonNodes before Init");
		static_assert(sizeof(SkeletonNode) == 32, "a node record is 32 bytes");
		const size_t bytes = dxv_skeleton_nodes_bytes(m_ctx);
		nodes.resize(bytes / sizeof(SkeletonNode));
		return dxv_skeleton_nodes_download(m_ctx, nodes.data(), bytes) == 0;
	}
	bool SkeletonBranches(std::vector<SkeletonBranch>& branches)
	{
		if (!m_ctx) return setError("SkeletonBranches before Init");
		static_assert(sizeof(SkeletonBranch) == 48, "a branch record is 48 bytes");
		const size_t bytes = dxv_skeleton_branches_bytes(m_ctx);
		branches.resize(bytes / sizeof(SkeletonBranch));
		return dxv_skeleton_branches_download(m_ctx, branches.data(), bytes) == 0;
	}
	bool SkeletonInfo(SkeletonCounts& c)
	{
		return m_ctx && dxv_skeleton_info(m_ctx, &c.ms, &c.nodes, &c.branches, &c.endVoxels, &c.curveVoxels, &c.junctionVoxels) == 0;
	}
	bool SkeletonPrune(uint32_t maxLen345, bool sync = true) { return m_ctx && (sync ? dxv_skeleton_prune(m_ctx, maxLen345) : dxv_skeleton_prune_async(m_ctx, maxLen345)) == 0; }
	bool SkeletonPruneInfo(uint32_t& branchesRemoved, uint64_t& voxelsRemoved) { return m_ctx && dxv_skeleton_prune_info(m_ctx, &branchesRemoved, &voxelsRemoved) == 0; }
	static double SkeletonLength(const SkeletonBranch& b) { return b.steps[0] + 1.4142135623730951 * b.steps[1] + 1.7320508075688772 * b.steps[2]; }

	// The geodesic distance inside the selected frame's whole grid (dxv_geodesic / dxv_geodesic_async; include/dxv.h has the rule): per member voxel
	// the length of the shortest path of member voxels to the nearest seed -- DXV_GEO_FACES over the face neighbours at weight 1, DXV_GEO_CHAMFER
	// over the 26 neighbours at weights 3 / 4 / 5 --, DXV_GEO_NONE on the others, DXV_GEO_UNREACHED where no path exists or is longer than limit
	// (0: no limit).  Seeds: the grid's border, a list of voxel indices, or a mask of N^3 bytes in device memory.  The grid and the frame's other
	// products stay as they are.
	bool Geodesic(int of = DXV_COMP_SOLID, int metric = DXV_GEO_CHAMFER, uint32_t limit = 0, bool sync = true)
	{
		return m_ctx && (sync ? dxv_geodesic(m_ctx, of, metric, DXV_GEO_SEEDS_BORDER, nullptr, 0, limit) : dxv_geodesic_async(m_ctx, of, metric, DXV_GEO_SEEDS_BORDER, nullptr, 0, limit)) == 0;
	}
	bool Geodesic(int of, int metric, const std::vector<uint32_t>& seeds, uint32_t limit = 0, bool sync = true)
	{
		const uint32_t count = static_cast<uint32_t>(seeds.size());
		return m_ctx && (sync ? dxv_geodesic(m_ctx, of, metric, DXV_GEO_SEEDS_LIST, seeds.data(), count, limit) : dxv_geodesic_async(m_ctx, of, metric, DXV_GEO_SEEDS_LIST, seeds.data(), count, limit)) == 0;
	}
	bool GeodesicFromDeviceMask(int of, int metric, const void* deviceMask, uint32_t limit = 0, bool sync = true)
	{
		return m_ctx && (sync ? dxv_geodesic(m_ctx, of, metric, DXV_GEO_SEEDS_MASK, deviceMask, 0, limit) : dxv_geodesic_async(m_ctx, of, metric, DXV_GEO_SEEDS_MASK, deviceMask, 0, limit)) == 0;
	}
	const void* DeviceGeodesic() const { return m_ctx ? dxv_geodesic_device_ptr(m_ctx) : nullptr; }
	bool GeodesicField(std::vector<uint32_t>& field)
	{
		if (!m_ctx) return setError("GeodesicField before Init");
		const size_t bytes = dxv_geodesic_bytes(m_ctx);
		if (!bytes) return false;
		field.resize(bytes / sizeof(uint32_t));
		return dxv_geodesic_download(m_ctx, field.data(), bytes) == 0;
	}
	struct GeodesicTally { float ms = 0.0f; uint32_t rounds = 0; uint64_t seedsUsed = 0, reached = 0, unreached = 0; uint32_t farthest = 0, farthestVoxel = 0xFFFFFFFFu; };
	bool GeodesicInfo(GeodesicTally& t)
	{
		return m_ctx && dxv_geodesic_info(m_ctx, &t.ms, &t.rounds, &t.seedsUsed, &t.reached, &t.unreached, &t.farthest, &t.farthestVoxel) == 0;
	}
	// a shortest path from target down to a seed, as voxel indices (dxv_geodesic_path; synchronous)
	bool GeodesicPath(uint32_t target, std::vector<uint32_t>& path)
	{
		uint32_t length = 0;
		if (!m_ctx || dxv_geodesic_path(m_ctx, target, nullptr, 0, &length)) return false;
		path.resize(length);
		return dxv_geodesic_path(m_ctx, target, path.data(), length, &length) == 0 && length == path.size();
	}

	// What can get in (dxv_access / dxv_access_async; include/dxv.h has the rule): per member voxel the access map A -- the squared radius of the
	// largest voxel-centred ball whose centre can travel from a seed to the voxel without leaving the members, steps over the 6 or the 26
	// neighbours -- and with intrusion the intrusion map I, the largest such ball that covers the voxel; 0 elsewhere and where nothing gets to.
	// Seeds as for Geodesic.  sync = false only enqueues one batch of rounds: the intrusion map is made where the frame is next synchronised.
	bool Access(int of = DXV_COMP_EMPTY, int connectivity = 26, uint32_t capSq = 4096, bool intrusion = true, bool sync = true)
	{
		return m_ctx && (sync ? dxv_access(m_ctx, of, connectivity, capSq, DXV_GEO_SEEDS_BORDER, nullptr, 0, intrusion) : dxv_access_async(m_ctx, of, connectivity, capSq, DXV_GEO_SEEDS_BORDER, nullptr, 0, intrusion)) == 0;
	}
	bool Access(int of, int connectivity, uint32_t capSq, const std::vector<uint32_t>& seeds, bool intrusion = true, bool sync = true)
	{
		const uint32_t count = static_cast<uint32_t>(seeds.size());
		return m_ctx && (sync ? dxv_access(m_ctx, of, connectivity, capSq, DXV_GEO_SEEDS_LIST, seeds.data(), count, intrusion) : dxv_access_async(m_ctx, of, connectivity, capSq, DXV_GEO_SEEDS_LIST, seeds.data(), count, intrusion)) == 0;
	}
	bool AccessFromDeviceMask(int of, int connectivity, uint32_t capSq, const void* deviceMask, bool intrusion = true, bool sync = true)
	{
		return m_ctx && (sync ? dxv_access(m_ctx, of, connectivity, capSq, DXV_GEO_SEEDS_MASK, deviceMask, 0, intrusion) : dxv_access_async(m_ctx, of, connectivity, capSq, DXV_GEO_SEEDS_MASK, deviceMask, 0, intrusion)) == 0;
	}
	const void* DeviceAccess() const { return m_ctx ? dxv_access_device_ptr(m_ctx) : nullptr; }
	const void* DeviceIntrusion() const { return m_ctx ? dxv_intrusion_device_ptr(m_ctx) : nullptr; }
	bool AccessField(std::vector<uint32_t>& field)
	{
		if (!m_ctx) return setError("AccessField before Init");
		const size_t bytes = dxv_access_bytes(m_ctx);
		if (!bytes) return false;
		field.resize(bytes / sizeof(uint32_t));
		return dxv_access_download(m_ctx, field.data(), bytes) == 0;
	}
	bool AccessHistogram(std::vector<uint64_t>& histogram)
	{
		if (!m_ctx) return setError("AccessHistogram before Init");
		const size_t bytes = dxv_access_histogram_bytes(m_ctx);
		if (!bytes) return false;
		histogram.resize(bytes / sizeof(uint64_t));
		return dxv_access_histogram_download(m_ctx, histogram.data(), bytes) == 0;
	}
	bool IntrusionField(std::vector<uint32_t>& field)
	{
		if (!m_ctx) return setError("IntrusionField before Init");
		const size_t bytes = dxv_intrusion_bytes(m_ctx);
		if (!bytes) return false;
		field.resize(bytes / sizeof(uint32_t));
		return dxv_intrusion_download(m_ctx, field.data(), bytes) == 0;
	}
	bool IntrusionHistogram(std::vector<uint64_t>& histogram)
	{
		if (!m_ctx) return setError("IntrusionHistogram before Init");
		const size_t bytes = dxv_intrusion_histogram_bytes(m_ctx);
		if (!bytes) return false;
		histogram.resize(bytes / sizeof(uint64_t));
		return dxv_intrusion_histogram_download(m_ctx, histogram.data(), bytes) == 0;
	}
	struct AccessTally { float ms = 0.0f; uint32_t rounds = 0; uint64_t seedsUsed = 0, reached = 0, unreached = 0; uint32_t widest = 0, widestVoxel = 0xFFFFFFFFu; };
	bool AccessInfo(AccessTally& t)
	{
		return m_ctx && dxv_access_info(m_ctx, &t.ms, &t.rounds, &t.seedsUsed, &t.reached, &t.unreached, &t.widest, &t.widestVoxel) == 0;
	}

	// What a straight line reaches (dxv_sight / dxv_sight_async; include/dxv.h has the rule): per voxel a uint32 with bit SightBit(dx, dy, dz) set
	// when the voxel is a member and every voxel behind it against the direction, up to the grid's border, is one too.  directions: a non-empty
	// subset of DXV_SIGHT_ALL.  Refers to the frame last selected; sync = false only enqueues (WaitFrame reports).
	static uint32_t SightBit(int dx, int dy, int dz) { return (uint32_t)((dz + 1) * 9 + (dy + 1) * 3 + (dx + 1)); }
	bool Sight(int of = DXV_COMP_EMPTY, uint32_t directions = DXV_SIGHT_ALL, bool sync = true)
	{
		return m_ctx && (sync ? dxv_sight(m_ctx, of, directions) : dxv_sight_async(m_ctx, of, directions)) == 0;
	}
	const void* DeviceSight() const { return m_ctx ? dxv_sight_device_ptr(m_ctx) : nullptr; }
	bool SightField(std::vector<uint32_t>& field)
	{
		if (!m_ctx) return setError("SightField before Init");
		const size_t bytes = dxv_sight_bytes(m_ctx);
		if (!bytes) return false;
		field.resize(bytes / sizeof(uint32_t));
		return dxv_sight_download(m_ctx, field.data(), bytes) == 0;
	}
	// the tally: the members, those seen along each direction's bit, per axis asked for both ways those seen along neither of its directions,
	// and count[k] those seen along exactly k of the requested directions
	struct SightCounts { uint64_t members = 0, seen[27] = {}, neither[13] = {}, count[27] = {}; };
	bool SightTally(SightCounts& t) { return m_ctx && dxv_sight_tally_download(m_ctx, &t, sizeof(t)) == 0; }
	bool SightInfo(float& ms, int& of, uint32_t& directions) { return m_ctx && dxv_sight_info(m_ctx, &ms, &of, &directions) == 0; }
	// the axis (0 .. 12, direction bit 14 + axis) with the fewest members seen along neither of its directions: the best pull axis
	static int BestSightAxis(const SightCounts& t)
	{
		int best = 0;
		for (int a = 1; a < 13; ++a)
			if (t.neither[a] < t.neither[best]) best = a;
		return best;
	}
	// The edit from that map, in place (dxv_sight_fill / dxv_sight_fill_async): every member seen along none of `directions` changes kind.
	bool SightFill(uint32_t directions, bool sync = true) { return m_ctx && (sync ? dxv_sight_fill(m_ctx, directions) : dxv_sight_fill_async(m_ctx, directions)) == 0; }

	// The exterior flood fill of that frame's whole grid, in place (dxv_fill / dxv_fill_async): DXV_FILL_SOLID leaves the walls and everything
	// they enclose, DXV_FILL_INTERIOR the enclosed voxels alone.  Voxelize(gridDim, SURFACE) && Fill() is the solid of a mesh whose
	// normals and watertightness cannot be trusted.  Refers to the frame last selected; sync = false only enqueues (WaitFrame reports).
	bool Fill(int what = DXV_FILL_SOLID, bool sync = true) { return m_ctx && (sync ? dxv_fill(m_ctx, what) : dxv_fill_async(m_ctx, what)) == 0; }
	bool FillInfo(float& ms, uint32_t& rounds) { return m_ctx && dxv_fill_info(m_ctx, &ms, &rounds) == 0; }
	// That frame's solid grown or shrunk by the Euclidean ball of squared radius radiusSq (1 .. 4096), in place (dxv_morph / dxv_morph_async):
	// DXV_MORPH_DILATE, _ERODE, _OPEN, _CLOSE.  Voxelize(gridDim, SURFACE) && Morph(DXV_MORPH_DILATE, r2) && Fill() && Morph(DXV_MORPH_ERODE, r2)
	// is the solid of a mesh with holes narrower than the ball.
	bool Morph(int op, uint32_t radiusSq, bool sync = true) { return m_ctx && (sync ? dxv_morph(m_ctx, op, radiusSq) : dxv_morph_async(m_ctx, op, radiusSq)) == 0; }
	bool MorphInfo(float& ms, uint64_t& voxelsSet, uint64_t& voxelsCleared) { return m_ctx && dxv_morph_info(m_ctx, &ms, &voxelsSet, &voxelsCleared) == 0; }
	// That frame's solid thinned without a change of topology, in place (dxv_thin / dxv_thin_async): DXV_THIN_CURVE leaves a curve skeleton,
	// DXV_THIN_KERNEL the topological kernel; maxIterations = 0: to the fixed point.  Voxels outside the grid are empty.
	bool Thin(int kind, uint32_t maxIterations = 0, bool sync = true) { return m_ctx && (sync ? dxv_thin(m_ctx, kind, maxIterations) : dxv_thin_async(m_ctx, kind, maxIterations)) == 0; }
	bool ThinInfo(float& ms, uint32_t& iterations, uint64_t& voxelsRemoved, bool& converged)
	{
		int c = 0;
		const bool ok = m_ctx && dxv_thin_info(m_ctx, &ms, &iterations, &voxelsRemoved, &c) == 0;
		converged = c != 0;
		return ok;
	}

	// Result: uint8 occupancy, x fastest, then y (top to bottom), then z.
	bool Download(std::vector<uint8_t>& grid)
	{
		if (!m_ctx) return setError("Download before Init");
		grid.resize(dxv_grid_bytes(m_ctx));
		return dxv_grid_download(m_ctx, grid.data(), grid.size()) == 0;
	}
	// One bit per voxel (voxel 8j+i in bit i of byte j), packed on the device: 8x less PCIe traffic.
	bool DownloadBits(std::vector<uint8_t>& bits)
	{
		if (!m_ctx) return setError("DownloadBits before Init");
		bits.resize(dxv_grid_packed_bytes(m_ctx));
		return dxv_grid_download_packed(m_ctx, bits.data(), bits.size()) == 0;
	}
	const void* DeviceGrid() const { return m_ctx ? dxv_grid_device_ptr_ro(m_ctx) : nullptr; }
	bool CountSolid(uint64_t& solid) { return m_ctx && dxv_grid_count(m_ctx, &solid) == 0; }

	bool GetStats(dxv_stats& s) const { return m_ctx && dxv_get_stats(m_ctx, &s) == 0; }
	const char* LastError() const { return m_ctx && *dxv_last_error(m_ctx) ? dxv_last_error(m_ctx) : m_err.c_str(); }
	dxv_ctx* Context() { return m_ctx; }

	static const uint8_t FrameCount = DXV_FRAME_COUNT; // Content/Voxelizer.h:24: grids (frames) the component owns

protected:
	bool setError(const char* msg) { m_err = msg ? msg : ""; return false; }

	dxv_ctx*	m_ctx = nullptr;
	int			m_device;
	float		m_posScale[4] = { 0.0f, 0.0f, 0.0f, 1.0f };
	float		m_eyePt[3] = { 8.0f, 12.0f, -14.0f };	// DXRVoxelizer.cpp:230
	float		m_viewProj[16] = { 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1 };
	uint32_t	m_width = 1280, m_height = 720;	// Main.cpp:17
	std::string	m_err;
};
