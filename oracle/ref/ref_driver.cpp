// ref_driver.cpp — a caller of the reference's entry points, for fixtures.
// TEST INFRASTRUCTURE ONLY.  oracle/ref/build_ref.py compiles this file, with
// prelude.h force-included, into oracle/_ref/ref_driver; REF_HEADER and
// REF_SOURCE name the reference's header and the lane-rewritten copy of its
// source, which is included here so that its file-local functions can be
// called.  Nothing in this file comes from the reference.
//
//   ref_driver SCENE OUTPREFIX       draw the scene file, write OUTPREFIX.color
//                                    (u32), .z (f32), .winners (i32) and, on
//                                    request, .edges (28 words per edge)
//   ref_driver --sphere OUTPREFIX    ConstructSphere: .sphere (count, then
//                                    vertices, colours, normals, uvs)
//
// Every scene is drawn twice, with the memory around the texture (and the
// edge, sort and work arenas before use) filled with two different bytes; the
// texture's zeroed guard row stays.  The second frame is only compared with
// the first: the last line of output counts the pixels that differ, which are
// the pixels whose value depends on memory the reference does not own.
#include REF_HEADER
#include REF_SOURCE

#include <sys/mman.h>

#include <stdexcept>
#include <string>
#include <vector>

namespace {

enum { MODE_QUEUE = 0, MODE_SINGLE = 1, MODE_SCALAR = 2, MODE_LINES = 3 };
const u32 kMagic = 0x31464552u;  // "REF1"

struct scene_file {
    s32 W, H, Tris, TrisPerObject, Mode, Phong, TexW, TexH, LightCount, DumpEdges;
    r32 P[3], T[5], Ambient[4];
    std::vector<r32> Lights, V, C, N, UV;
    std::vector<u32> Texels;  // (TexH + 1) rows of TexW, the last one zero
};

void read_exact(FILE *f, void *p, size_t n) {
    if (n && fread(p, 1, n, f) != n) throw std::runtime_error("scene file too short");
}

scene_file load(const char *path) {
    FILE *f = fopen(path, "rb");
    if (!f) throw std::runtime_error("cannot open scene file");
    s32 h[16];
    read_exact(f, h, sizeof h);
    if ((u32)h[0] != kMagic) throw std::runtime_error("not a scene file");
    scene_file s;
    s.W = h[1]; s.H = h[2]; s.Tris = h[3]; s.TrisPerObject = h[4]; s.Mode = h[5]; s.Phong = h[6];
    s.TexW = h[7]; s.TexH = h[8]; s.LightCount = h[9]; s.DumpEdges = h[10];
    if (s.W <= 0 || s.W % 8 || s.H <= 0 || s.Tris <= 0 || s.TrisPerObject <= 0 || s.LightCount < 0 ||
        s.LightCount > 8 || s.TexW < 0 || s.TexH < 0 || s.Mode < 0 || s.Mode > MODE_LINES)
        throw std::runtime_error("scene header out of range (frame widths are multiples of 8)");
    read_exact(f, s.P, sizeof s.P);
    read_exact(f, s.T, sizeof s.T);
    read_exact(f, s.Ambient, sizeof s.Ambient);
    s.Lights.resize(7 * (size_t)s.LightCount);
    s.V.resize(9 * (size_t)s.Tris);
    s.C.resize(12 * (size_t)s.Tris);
    s.N.resize(9 * (size_t)s.Tris);
    s.UV.resize(6 * (size_t)s.Tris);
    read_exact(f, s.Lights.data(), 4 * s.Lights.size());
    read_exact(f, s.V.data(), 4 * s.V.size());
    read_exact(f, s.C.data(), 4 * s.C.size());
    read_exact(f, s.N.data(), 4 * s.N.size());
    read_exact(f, s.UV.data(), 4 * s.UV.size());
    if (s.TexW && s.TexH) {
        s.Texels.resize((size_t)(s.TexH + 1) * s.TexW);
        read_exact(f, s.Texels.data(), 4 * s.Texels.size());
    }
    fclose(f);
    return s;
}

void *aligned(size_t bytes) {
    void *p = aligned_alloc(64, (bytes + 63) & ~(size_t)63);
    if (!p) throw std::bad_alloc();
    return p;
}

struct frame {
    std::vector<u32> Color;
    std::vector<u32> Z;  // bit patterns
    std::vector<s32> Winners;
    std::vector<u32> Edges;  // 28 words per edge: the 27 non-pointer words, Next as an index (-1: null)
    u32 Skipped = 0;         // objects FillEdgeTable gave no edge (nothing drawn)
};

frame draw(const scene_file &s, u8 fill) {
    const size_t px = (size_t)s.W * s.H;
    u32 *color = (u32 *)aligned(px * 4);
    r32 *z = (r32 *)aligned(px * 4);
    const size_t zmask_bytes = px / 8 + 8;
    u8 *zmask = (u8 *)aligned(zmask_bytes);
    memset(zmask, 0, zmask_bytes);
    for (size_t i = 0; i < px; ++i) { color[i] = 0xFF000000u; z[i] = -3.402823466e+38f; }

    // The texture inside an arena of our own.  The reference forms a texel's
    // address from a signed 32-bit byte offset, for masked-out lanes from
    // whatever uv they extrapolate to, so the arena spans 2 GiB to either side
    // (reserved, never committed: untouched pages read as zero).  The near part
    // (pad, texels, zeroed guard row, pad) carries the fill byte.  Lanes the
    // AVX paths keep have uv in [0, 1] and read the near part only; DrawModel
    // masks nothing, so for it the far part is not readable at all.
    loaded_bitmap bitmap = {};
    u8 *arena = nullptr;
    size_t arena_bytes = 0;
    if (!s.Texels.empty()) {
        const size_t page = 4096, half = (size_t)1 << 31;
        const size_t tex_bytes = s.Texels.size() * 4;
        const size_t pad = (((size_t)1 << 20) + 16 * tex_bytes + page - 1) / page * page;
        const size_t near_bytes = (2 * pad + tex_bytes + page - 1) / page * page;
        arena_bytes = 2 * half + near_bytes;
        arena = (u8 *)mmap(nullptr, arena_bytes, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE,
                           -1, 0);
        if (arena == MAP_FAILED) throw std::runtime_error("cannot reserve the texture arena");
        u8 *near_part = arena + half;
        memset(near_part, fill, near_bytes);
        memcpy(near_part + pad, s.Texels.data(), tex_bytes);
        if (s.Mode == MODE_SCALAR) {
            mprotect(arena, half, PROT_NONE);
            mprotect(near_part + near_bytes, half, PROT_NONE);
        }
        bitmap.Memory = near_part + pad;
        bitmap.Width = s.TexW;
        bitmap.Height = s.TexH;
        bitmap.Pitch = s.TexW * BITMAP_BYTES_PER_PIXEL;
    }
    loaded_bitmap *Bitmap = arena ? &bitmap : 0;

    loaded_bitmap target = {color, s.W, s.H, s.W * BITMAP_BYTES_PER_PIXEL};

    const u32 max_edges = 3u * (u32)s.TrisPerObject;
    const size_t edge_bytes = (size_t)(max_edges + 1) * sizeof(edge_info);
    edge_info *edges = (edge_info *)aligned(edge_bytes);
    edge_info *sort = (edge_info *)aligned(edge_bytes);
    // every row may queue one record per pair of listed edges
    const size_t work_bytes = ((size_t)s.H + 1) * (max_edges + 2) * sizeof(line_render_work) + 4096;
    void *work = aligned(work_bytes);

    game_render_commands commands = {};
    commands.ZBuffer = z;
    commands.ZMask = zmask;
    commands.Width = (u32)s.W;
    commands.ThreadMemory = work;
    commands.ThreadMemorySize = (u32)(work_bytes > 0xFFFFFFFFu ? 0xFFFFFFFFu : work_bytes);
    commands.SortMemory = sort;
    commands.Transform.DistanceAboveTarget = s.T[0];
    commands.Transform.FocalLength = s.T[1];
    commands.Transform.MetersToPixels = s.T[2];
    commands.Transform.ScreenCenter = V2(s.T[3], s.T[4]);
    commands.LightData.LightCount = (u32)s.LightCount;
    commands.LightData.AmbientIntensity = V4(s.Ambient[0], s.Ambient[1], s.Ambient[2], s.Ambient[3]);
    for (s32 i = 0; i < s.LightCount; ++i) {
        const r32 *l = &s.Lights[7 * (size_t)i];
        commands.LightData.Lights[i].P = V3(l[0], l[1], l[2]);
        commands.LightData.Lights[i].Intensity = V4(l[3], l[4], l[5], l[6]);
    }
    platform_work_queue queue = {};

    frame out;
    out.Winners.assign(px, -1);
    std::vector<u32> color0(px), z0(px);

    for (s32 first = 0, obj = 0; first < s.Tris; first += s.TrisPerObject, ++obj) {
        const s32 tris = first + s.TrisPerObject <= s.Tris ? s.TrisPerObject : s.Tris - first;
        render_entry_3d_object object = {};
        object.P = V3(s.P[0], s.P[1], s.P[2]);
        object.VertexCount = 3u * (u32)tris;
        object.Optimized = s.Mode != MODE_SCALAR;
        object.PhongShading = s.Phong;
        object.VertexData = (void *)&s.V[9 * (size_t)first];
        object.ColorData = (void *)&s.C[12 * (size_t)first];
        object.NormalData = (void *)&s.N[9 * (size_t)first];
        object.UVData = (void *)&s.UV[6 * (size_t)first];
        object.EdgeMemory = edges;
        object.Bitmap = Bitmap;
        // fresh edge memory is zero (fields FillEdgeTable leaves alone read as
        // 0); the sort and work arenas are only ever read after being written
        memset(edges, 0, edge_bytes);
        memset(sort, fill, edge_bytes);
        WorkIndex = 0;
        commands.ThreadMemorySizeUsed = 0;

        // An object with no visible edge: the reference's sort asserts on a
        // count of 0 (prelude.h turns Assert into an exception).  Such an
        // object is counted and not drawn.
        u32 count = 0;
        try {
            count = FillEdgeTable(&object, &commands, s.Phong);
        } catch (const reference_assert &) {
            ++out.Skipped;
            continue;
        }
        if (count == 0) { ++out.Skipped; continue; }
        if (s.DumpEdges && obj == 0) {
            for (u32 e = 0; e < count; ++e) {
                u32 w[28];
                memcpy(w, &edges[e], 27 * 4);
                const s32 next = edges[e].Next ? (s32)(edges[e].Next - edges) : -1;
                memcpy(&w[27], &next, 4);
                out.Edges.insert(out.Edges.end(), w, w + 28);
            }
        }

        // Winners: what this submission wrote.  The reference only ever blends
        // a new pixel over the old one under its write mask, so the colour
        // buffer holds the complement of the frame while the object draws: a
        // written pixel shows as a changed z or a colour that is not the
        // complement; unwritten pixels get their colour back.
        memcpy(z0.data(), z, px * 4);
        for (size_t i = 0; i < px; ++i) { color0[i] = color[i]; color[i] = ~color[i]; }
        switch (s.Mode) {
        case MODE_QUEUE: DrawModelOptimized(&queue, &target, edges, count, &commands, Bitmap, s.Phong); break;
        case MODE_LINES: DrawModelOptimizedLines(&queue, &target, edges, count, &commands, Bitmap, s.Phong); break;
        case MODE_SINGLE: DrawModelOptimized(&target, edges, count, &commands, Bitmap, s.Phong); break;
        default: DrawModel(&target, edges, count, &commands, Bitmap, s.Phong); break;
        }
        const u32 *zb = (const u32 *)z;
        for (size_t i = 0; i < px; ++i) {
            if (zb[i] != z0[i] || color[i] != ~color0[i]) out.Winners[i] = first;  // patched below
            else color[i] = color0[i];
        }
    }
    // Winners per triangle: an object's pixels carry its first triangle; for
    // one-triangle objects that is the triangle itself.
    out.Color.assign(color, color + px);
    out.Z.assign((const u32 *)z, (const u32 *)z + px);
    free(color); free(z); free(zmask); free(edges); free(sort); free(work);
    if (arena) munmap(arena, arena_bytes);
    return out;
}

void write_file(const std::string &path, const void *p, size_t bytes) {
    FILE *f = fopen(path.c_str(), "wb");
    if (!f || (bytes && fwrite(p, 1, bytes, f) != bytes)) throw std::runtime_error("cannot write " + path);
    fclose(f);
}

int sphere(const std::string &prefix) {
    const u32 cap = 3 * 2 * 24 * 48 + 64;  // two triangles per cell of a 24 x 48 grid, and slack
    std::vector<v3> V(cap), N(cap);
    std::vector<v4> C(cap);
    std::vector<v2> UV(cap);
    const u32 n = ConstructSphere(V.data(), C.data(), N.data(), UV.data());
    if (n > cap) throw std::runtime_error("sphere larger than expected");
    FILE *f = fopen((prefix + ".sphere").c_str(), "wb");
    if (!f) throw std::runtime_error("cannot write sphere");
    fwrite(&n, 4, 1, f);
    fwrite(V.data(), sizeof(v3), n, f);
    fwrite(C.data(), sizeof(v4), n, f);
    fwrite(N.data(), sizeof(v3), n, f);
    fwrite(UV.data(), sizeof(v2), n, f);
    fclose(f);
    printf("sphere vertices=%u\n", n);
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    try {
        if (argc == 3 && !strcmp(argv[1], "--sphere")) return sphere(argv[2]);
        if (argc != 3) {
            fprintf(stderr, "usage: ref_driver SCENE OUTPREFIX | --sphere OUTPREFIX\n");
            return 2;
        }
        const scene_file s = load(argv[1]);
        const frame a = draw(s, 0x5A), b = draw(s, 0xA5);
        size_t undefined = 0;
        for (size_t i = 0; i < a.Color.size(); ++i)
            undefined += a.Color[i] != b.Color[i] || a.Z[i] != b.Z[i] || a.Winners[i] != b.Winners[i];
        const std::string prefix = argv[2];
        write_file(prefix + ".color", a.Color.data(), a.Color.size() * 4);
        write_file(prefix + ".z", a.Z.data(), a.Z.size() * 4);
        write_file(prefix + ".winners", a.Winners.data(), a.Winners.size() * 4);
        if (s.DumpEdges) write_file(prefix + ".edges", a.Edges.data(), a.Edges.size() * 4);
        printf("objects_without_edges=%u undefined_pixels=%zu\n", a.Skipped, undefined);
        return 0;
    } catch (const reference_assert &e) {
        fprintf(stderr, "ref_driver: reference Assert failed at line %d of the rewritten source\n", e.Line);
        return 3;
    } catch (const std::exception &e) {
        fprintf(stderr, "ref_driver: %s\n", e.what());
        return 2;
    }
}
