// dxv_blob.hip -- the built scene as one relocatable device blob (what rank 0 broadcasts to the other GPUs): layout, export,
// checksum, import with validation of everything the kernels will index with.
#include "dxv_ctx.h"

using namespace dxv;
using namespace dxvhost;

namespace {
// an exported blob = the scene as it lies in memory + (when the context has built them) the lists' two arrays
struct BlobLayout { size_t offCells, cellBytes, offEntries, entryBytes, offPlCells, plCellBytes, offPlEntries, plEntryBytes, total; };
BlobLayout blob_layout(size_t sceneBytes, uint32_t listRes, uint32_t listCount, uint32_t plRes, uint32_t plCount)
{
    BlobLayout b{0, 0, 0, 0, 0, 0, 0, 0, sceneBytes};
    if (listRes) {
        b.offCells = align256(b.total);
        b.cellBytes = sizeof(DirCell) * 6 * (size_t)listRes * listRes;
        b.offEntries = align256(b.offCells + b.cellBytes);
        b.entryBytes = sizeof(DirEntry) * (size_t)listCount;
        b.total = align256(b.offEntries + b.entryBytes);
    }
    if (plRes) {
        b.offPlCells = align256(b.total);
        b.plCellBytes = sizeof(uint32_t) * 2 * (size_t)plRes * plRes;
        b.offPlEntries = align256(b.offPlCells + b.plCellBytes);
        b.plEntryBytes = sizeof(uint32_t) * (size_t)plCount;
        b.total = align256(b.offPlEntries + b.plEntryBytes);
    }
    return b;
}
bool lists_exportable(const dxv_ctx* c) { return c->lists.state == 1 && c->lists.opt == c->opt.listres; }
bool plists_exportable(const dxv_ctx* c) { return c->rowLists.state == 1 && (c->opt.plistres == 0 || (uint32_t)c->opt.plistres == c->rowLists.res); }
BlobLayout export_layout(const dxv_ctx* c)
{
    const bool l = lists_exportable(c), pl = plists_exportable(c);
    return blob_layout(c->sceneBytes, l ? c->lists.res : 0u, l ? c->lists.count : 0u, pl ? c->rowLists.res : 0u, pl ? c->rowLists.count : 0u);
}
} // namespace

extern "C" {

size_t dxv_scene_bytes(const dxv_ctx* c)
{
    if (!c || !c->haveScene) return 0;
    return export_layout(c).total;
}

int dxv_scene_export(dxv_ctx* c, void* dst, size_t bytes)
{
    if (!c) return 1;
    if (!c->haveScene) return fail(c, "dxv_scene_export: no scene");
    if (settle_lists(c)) return 1;
    const bool withLists = lists_exportable(c), withPl = plists_exportable(c);
    const BlobLayout b = export_layout(c);
    if (!dst || bytes != b.total) return fail(c, "dxv_scene_export: expected %zu bytes, got %zu", b.total, bytes);
    DXV_HIP(c, hipSetDevice(c->device));
    if (ensure_nodes(c, c->stream)) return 1;
    DXV_HIP(c, hipMemcpyAsync(dst, c->scene.p, c->sceneBytes, hipMemcpyDeviceToDevice, c->stream));
    SceneHeader h = c->hdr;
    h.offListCells = h.offListEntries = 0; h.listRes = h.listCount = 0;
    h.offPlCells = h.offPlEntries = 0; h.plRes = h.plCount = 0;
    uint8_t* out = static_cast<uint8_t*>(dst);
    if (withLists) {
        DXV_HIP(c, hipMemcpyAsync(out + b.offCells, c->lists.cells.p, b.cellBytes, hipMemcpyDeviceToDevice, c->stream));
        if (b.entryBytes) DXV_HIP(c, hipMemcpyAsync(out + b.offEntries, c->lists.entries.p, b.entryBytes, hipMemcpyDeviceToDevice, c->stream));
        h.offListCells = b.offCells; h.offListEntries = b.offEntries; h.listRes = c->lists.res; h.listCount = c->lists.count;
    }
    if (withPl) {
        DXV_HIP(c, hipMemcpyAsync(out + b.offPlCells, c->rowLists.cells.p, b.plCellBytes, hipMemcpyDeviceToDevice, c->stream));
        if (b.plEntryBytes) DXV_HIP(c, hipMemcpyAsync(out + b.offPlEntries, c->rowLists.entries.p, b.plEntryBytes, hipMemcpyDeviceToDevice, c->stream));
        h.offPlCells = b.offPlCells; h.offPlEntries = b.offPlEntries; h.plRes = c->rowLists.res; h.plCount = c->rowLists.count;
    }
    h.totalBytes = b.total;
    DXV_HIP(c, hipMemcpyAsync(dst, &h, sizeof(h), hipMemcpyHostToDevice, c->stream));     // the blob's own header (the resident one keeps the scene's size)
    DXV_HIP(c, hipStreamSynchronize(c->stream));
    return 0;
}

int dxv_scene_checksum(dxv_ctx* c, const void* device_blob, size_t bytes, uint64_t* sum)
{
    if (!c || !sum) return 1;
    if (!device_blob || bytes < 8) return fail(c, "dxv_scene_checksum: no blob");
    DXV_HIP(c, hipSetDevice(c->device));
    DXV_HIP(c, launch_checksum(device_blob, bytes, c->count.p, c->stream));
    unsigned long long v = 0;
    DXV_HIP(c, hipMemcpyAsync(&v, c->count.p, sizeof(v), hipMemcpyDeviceToHost, c->stream));
    DXV_HIP(c, hipStreamSynchronize(c->stream));
    *sum = v;
    return 0;
}

int dxv_scene_import(dxv_ctx* c, const void* src, size_t bytes)
{
    if (!c) return 1;
    if (!src || bytes < sizeof(SceneHeader)) return fail(c, "dxv_scene_import: blob too small (%zu bytes)", bytes);
    DXV_HIP(c, hipSetDevice(c->device));
    SceneHeader h;
    DXV_HIP(c, hipMemcpyAsync(&h, src, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    DXV_HIP(c, hipStreamSynchronize(c->stream));
    if (h.magic != kSceneMagic || h.version != kSceneVersion) return fail(c, "dxv_scene_import: bad magic/version");
    SceneHeader want;
    layout_scene(want, h.numTris, h.numVerts, h.hasWide != 0);
    const bool withLists = h.listRes != 0;
    if (withLists && (h.listRes < 16u || h.listRes > 4096u || (h.listRes & (h.listRes - 1u)) || h.listCount > 0x7fffffffu))
        return fail(c, "dxv_scene_import: inconsistent list section (res=%u, entries=%u)", h.listRes, h.listCount);
    const bool withPl = h.plRes != 0;
    if (withPl && (h.plRes < 16u || h.plRes > 4096u || (h.plRes & (h.plRes - 1u)) || h.plCount > 0x7ffffff0u))
        return fail(c, "dxv_scene_import: inconsistent row-list section (res=%u, entries=%u)", h.plRes, h.plCount);
    const BlobLayout b = blob_layout(want.totalBytes, withLists ? h.listRes : 0u, withLists ? h.listCount : 0u, withPl ? h.plRes : 0u, withPl ? h.plCount : 0u);
    if (!h.numTris || b.total != bytes || h.totalBytes != bytes || h.offNodes != want.offNodes ||
        h.offTriPos != want.offTriPos || h.offTriNrm != want.offTriNrm || h.offNodes32 != want.offNodes32 || h.offNodes64 != want.offNodes64 || h.hasWide > 1u || h.treeHeight == 0 || h.treeHeight > 64 ||
        (withLists && (h.offListCells != b.offCells || h.offListEntries != b.offEntries)) || (!withLists && (h.offListCells || h.offListEntries || h.listCount)) ||
        (withPl && (h.offPlCells != b.offPlCells || h.offPlEntries != b.offPlEntries)) || (!withPl && (h.offPlCells || h.offPlEntries || h.plCount)))
        return fail(c, "dxv_scene_import: inconsistent header (T=%u, bytes=%zu)", h.numTris, bytes);
    if (sync_frames(c)) return 1;
    scene_changed(c, SceneCause::import);
    // An imported scene carries no mesh and no build state: drop what an earlier dxv_set_mesh / dxv_build left on this
    // context, so that dxv_build, dxv_refit and dxv_update_vertices fail cleanly instead of running the imported
    // triangle count over the old, smaller buffers.
    DXV_HIP(c, hipStreamSynchronize(c->stream));
    c->vb.release(); c->ib.release();
    c->scratch = BuildScratch{};
    if (alloc_scene(c, h.numTris, h.numVerts, h.hasWide != 0)) return 1;
    DXV_HIP(c, hipMemcpyAsync(c->scene.p, src, want.totalBytes, hipMemcpyDeviceToDevice, c->stream));
    if (withLists) {
        // the lists travel with the scene: adopt them instead of building them again (1-5 ms per rank at 1 M triangles)
        DXV_HIP(c, c->lists.reserve(h.listRes, h.listCount));
        const uint8_t* in = static_cast<const uint8_t*>(src);
        DXV_HIP(c, hipMemcpyAsync(c->lists.cells.p, in + b.offCells, b.cellBytes, hipMemcpyDeviceToDevice, c->stream));
        if (b.entryBytes) DXV_HIP(c, hipMemcpyAsync(c->lists.entries.p, in + b.offEntries, b.entryBytes, hipMemcpyDeviceToDevice, c->stream));
        // The kernel indexes the entries with what the cells say and the triangle records with what the entries say: a blob
        // whose header is consistent but whose payload is not (cut short, corrupted, another version's) must not get that far.
        uint32_t bad[2] = {0, 0};
        DXV_HIP(c, dirmap_validate(c->lists.cells.p, h.listRes, c->lists.entries.p, h.listCount, h.numTris, c->rootInfo.p, c->stream));
        DXV_HIP(c, hipMemcpyAsync(bad, c->rootInfo.p, sizeof(bad), hipMemcpyDeviceToHost, c->stream));
        DXV_HIP(c, hipStreamSynchronize(c->stream));
        if (bad[0] || bad[1])
            return fail(c, "dxv_scene_import: the list section is inconsistent (%u texels point outside the %u entries, %u entries name a triangle >= %u)",
                        bad[0], h.listCount, bad[1], h.numTris);
        // the max-mip of the far radii is a function of the cells: made here, not carried in the blob
        DXV_HIP(c, dirmap_mip(c->lists.cells.p, h.listRes, c->lists.mip.p, c->stream));
        // ... and so are the start table and the start cells (of the validated cells and entries)
        DXV_HIP(c, dirmap_starts(c->lists.cells.p, h.listRes, c->lists.entries.p, c->lists.starts.p, c->lists.startCells.p, c->stream));
        DXV_HIP(c, hipMemcpyAsync(c->pin->listStarts, c->lists.starts.p + 6 * (size_t)h.listRes * h.listRes, sizeof(c->pin->listStarts), hipMemcpyDeviceToHost, c->stream));
        DXV_HIP(c, hipStreamSynchronize(c->stream));
        c->lists.startsPay = start_table_pays(c->pin->listStarts[0], c->pin->listStarts[1]);
    }
    if (withPl) {
        // ... and so do the row lists of the parity rule (1.6 ms per rank at 1 M triangles)
        DXV_HIP(c, c->rowLists.reserve(h.plRes, h.plCount));
        const uint8_t* in = static_cast<const uint8_t*>(src);
        DXV_HIP(c, hipMemcpyAsync(c->rowLists.cells.p, in + b.offPlCells, b.plCellBytes, hipMemcpyDeviceToDevice, c->stream));
        if (b.plEntryBytes) DXV_HIP(c, hipMemcpyAsync(c->rowLists.entries.p, in + b.offPlEntries, b.plEntryBytes, hipMemcpyDeviceToDevice, c->stream));
        DXV_HIP(c, hipMemsetAsync(c->rowLists.entries.p + h.plCount, 0, 8 * sizeof(uint32_t), c->stream));       // (the kernel fetches up to three slots behind a list)
        uint32_t bad[2] = {0, 0};
        DXV_HIP(c, parity_lists_validate(c->rowLists.cells.p, h.plRes, c->rowLists.entries.p, h.plCount, h.numTris, c->rootInfo.p, c->stream));
        DXV_HIP(c, hipMemcpyAsync(bad, c->rootInfo.p, sizeof(bad), hipMemcpyDeviceToHost, c->stream));
        DXV_HIP(c, hipStreamSynchronize(c->stream));
        if (bad[0] || bad[1])
            return fail(c, "dxv_scene_import: the row-list section is inconsistent (%u texels point outside the %u entries, %u entries name a triangle >= %u)",
                        bad[0], h.plCount, bad[1], h.numTris);
    }
    const uint32_t listRes = h.listRes, listCount = h.listCount, plRes = h.plRes, plCount = h.plCount;
    h.offListCells = h.offListEntries = 0; h.listRes = h.listCount = 0; h.totalBytes = want.totalBytes;   // the resident header describes the resident scene
    h.offPlCells = h.offPlEntries = 0; h.plRes = h.plCount = 0;
    DXV_HIP(c, hipMemcpyAsync(c->scene.p, &h, sizeof(h), hipMemcpyHostToDevice, c->stream));
    DXV_HIP(c, hipStreamSynchronize(c->stream));
    c->hdr = h;
    c->T = h.numTris; c->V = h.numVerts;
    memcpy(c->bound, h.bound, sizeof(c->bound));
    c->haveScene = true;
    ++c->sceneEpoch;
    if (withLists && (c->opt.listres == 0 || (uint32_t)c->opt.listres == listRes)) {   // (an explicit listres of another size: built here as asked)
        c->lists.count = listCount; c->lists.res = listRes; c->lists.state = 1; c->lists.opt = c->opt.listres; c->lists.ms = 0.0f;
        ++c->listEpoch;
    }
    if (withPl && (c->opt.plistres == 0 || (uint32_t)c->opt.plistres == plRes)) {
        c->rowLists.count = plCount; c->rowLists.res = plRes; c->rowLists.state = 1; c->rowLists.ms = 0.0f;
    }
    c->stackNow = initial_stack(c);
    fill_scene_stats(c);
    return 0;
}

} // extern "C"
