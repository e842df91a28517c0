"""Render the 12-ball array scene (the shape of matpreview/disney_bsdf_array0_envmap.xml) with a MaterialTable; with --scene, the
materials, layout and camera of a reference scene file, and with --analytic its bsdf_N balls under their analytic ground truth and
their own albedo."""
import sys, os, time, json, argparse
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from bsdf_diffusion_sampling_amd import wavefront as WF, weights as W
from bsdf_diffusion_sampling_amd.materials import MaterialTable
from bsdf_diffusion_sampling_amd.render_cli import write_png, tonemap
ap = argparse.ArgumentParser()
ap.add_argument("--width", type=int, default=683); ap.add_argument("--height", type=int, default=512)
ap.add_argument("--passes", type=int, default=64); ap.add_argument("--spp", type=int, default=4)
ap.add_argument("--domain", default="disk"); ap.add_argument("--measured-dir", default=None)
ap.add_argument("--out", default="gpurun_out/array0")
ap.add_argument("--max-depth", type=int, default=None, help="path vertices (PathArrayRenderer; default: ArrayRenderer's one bounce); "
                                                            "-1: unbounded, which needs --rr-depth")
ap.add_argument("--rr-depth", type=int, default=None, metavar="R",
                help="Russian roulette from the R-th vertex on (Mitsuba's rule; its default is 5).  Default: none")
ap.add_argument("--compact", action="store_true",
                help="run the bounces behind the first on the live-lane list of the bounce before (PathArrayRenderer(compact=True); "
                     "with --mesh-file: mesh.CompactMeshPathArrayRenderer): the same image bit for bit")
ap.add_argument("--transmission", action="store_true",
                help="follow BSDF samples below the surface through the balls (PathArrayRenderer(transmission=True)): needs "
                     "--scene with --analytic, --max-depth > 1 (or -1) and balls that touch neither each other nor the floor")
ap.add_argument("--integrator-from", default=None, metavar="scene.xml",
                help="--max-depth and --rr-depth from the <integrator> of a reference scene file (maxDepth = 2 is --max-depth 1, "
                     "-1 is unbounded; rrDepth defaults to 5); either option given explicitly wins")
ap.add_argument("--occlusion", type=int, choices=(0, 1), default=None, help="trace shadow rays (default: on when --max-depth > 1)")
ap.add_argument("--point-light", action="append", default=[], metavar="x,y,z:I",
                help="a point emitter at (x, y, z) (y up) of radiant intensity I (or r,g,b); repeatable, 8 at most "
                     "(a negative x needs the form --point-light=-1,4,2:200)")
ap.add_argument("--lights-from", default=None, metavar="scene.xml",
                help="the <emitter type=\"point\"> elements of a reference scene file (matpreview/disney_bsdf_array*_pointlight*.xml). "
                     "Its maxDepth = 2 (direct light only) is --max-depth 1 --occlusion 1 here: Mitsuba counts segments, this "
                     "renderer counts vertices; its unbounded depth is --max-depth -1 --rr-depth 5 (or --integrator-from)")
ap.add_argument("--no-env", action="store_true", help="with lights: a black environment that is no emitter (default: the sky emits too)")
ap.add_argument("--env-sampling", choices=("cosine", "importance"), default="cosine",
                help="the light strategy towards the environment: a cosine-weighted draw (default), or in proportion to the map's "
                     "luminance, as the reference's envmap emitter draws (PathArrayRenderer)")
ap.add_argument("--scene", default=None, metavar="scene.xml",
                help="materials, ball layout and camera from a reference scene file (wavefront.scene_from_matpreview_xml) in place "
                     "of the array0 scene; `mybsdf idx = N` balls use the shipped spherical nets bsdf_N")
ap.add_argument("--analytic", action="store_true",
                help="with --scene: shade the bsdf_N balls with their analytic ground truth (analytic.ground_truth_for) and give "
                     "every ball the albedo vector the file gives it (wavefront.albedos_from_matpreview_xml)")
ap.add_argument("--mesh-file", default=None, metavar="matpreview.serialized",
                help="with --scene: render the file's own geometry — its 25 instances of the three meshes of this container, under "
                     "their toWorld, and its lookAt camera — instead of twelve spheres on a plane: through mesh.MeshArrayRenderer (one "
                     "bounce, unoccluded), or, with any of --max-depth, --occlusion, --rr-depth, --integrator-from, --point-light, "
                     "--lights-from, --no-env, --compact, through mesh.MeshPathArrayRenderer (--compact: "
                     "mesh.CompactMeshPathArrayRenderer, the same image bit for bit).  No --transmission or --env-sampling "
                     "importance on meshes yet; parity-unpinned against Mitsuba")
a = ap.parse_args()
if a.analytic and not a.scene:
    ap.error("--analytic needs --scene")
if a.mesh_file and not a.scene:
    ap.error("--mesh-file needs --scene")
unbounded = a.max_depth == -1
if a.integrator_from:
    from bsdf_diffusion_sampling_amd.pathtrace import integrator_from_matpreview_xml
    xml_depth, xml_rr = integrator_from_matpreview_xml(a.integrator_from)
    if a.max_depth is None:
        a.max_depth, unbounded = xml_depth, xml_depth is None
    if a.rr_depth is None:
        a.rr_depth = xml_rr
if unbounded and a.rr_depth is None:
    ap.error("--max-depth -1 (unbounded) needs --rr-depth")
lights = []
if a.lights_from or a.point_light:
    from bsdf_diffusion_sampling_amd.pathtrace import PointLight, lights_from_matpreview_xml
    lights = lights_from_matpreview_xml(a.lights_from) if a.lights_from else []
    for spec in a.point_light:
        pos, _, inten = spec.partition(":")
        rgb = [float(v) for v in inten.split(",")]
        lights.append(PointLight(tuple(float(v) for v in pos.split(",")), rgb[0] if len(rgb) == 1 else tuple(rgb)))
if a.no_env and not lights:
    ap.error("--no-env needs --point-light or --lights-from")
mesh_scene = None
if a.mesh_file:
    from bsdf_diffusion_sampling_amd import mesh as MESH
    materials, cam, mesh_scene, _ = MESH.mesh_scene_from_matpreview_xml(a.scene, a.mesh_file, a.width, a.height)
    stems = [m + "_spherical" if m.startswith("bsdf_") else m + "_" + a.domain for m in materials]
elif a.scene:
    materials, cam, centers, radii = WF.scene_from_matpreview_xml(a.scene, a.width, a.height)
    stems = [m + "_spherical" if m.startswith("bsdf_") else m + "_" + a.domain for m in materials]
else:
    materials = WF.ARRAY0_MATERIALS
    cam, centers, radii = WF.array0_scene(a.width, a.height)
    stems = [m + "_" + a.domain for m in materials]
tab = MaterialTable(stems)
gts, extra = {}, {}
if a.analytic:
    from bsdf_diffusion_sampling_amd.analytic import ground_truth_for
    gts = ground_truth_for(materials)
    if len(gts) == len(materials):      # (a per-ball albedo needs ground truth on every ball)
        extra["ball_albedo"] = WF.albedos_from_matpreview_xml(a.scene)
elif a.measured_dir:
    from bsdf_diffusion_sampling_amd.measured import MeasuredBSDF, find_measured_file
    for i, m in enumerate(materials):
        p = find_measured_file(m, a.measured_dir)
        if p: gts[i] = MeasuredBSDF(p)
if a.env_sampling == "importance" and a.no_env:
    ap.error("--env-sampling importance needs an emitting environment: drop --no-env")
if mesh_scene is not None:
    if a.env_sampling != "cosine" or a.transmission:
        ap.error("--transmission and --env-sampling importance are not on meshes yet")
    if a.max_depth is None and not unbounded and a.rr_depth is None and a.occlusion is None and not lights and not a.compact:
        r = MESH.MeshArrayRenderer(tab, mesh_scene, camera=cam, ground_truth=gts, **extra)
    else:
        cls = MESH.CompactMeshPathArrayRenderer if a.compact else MESH.MeshPathArrayRenderer
        r = cls(tab, mesh_scene, camera=cam, ground_truth=gts, **extra,
                max_depth=None if unbounded else 1 if a.max_depth is None else a.max_depth, rr_depth=a.rr_depth,
                occlusion=None if a.occlusion is None else bool(a.occlusion), lights=lights,
                env=None if a.no_env or not lights else WF.make_sky())
elif (a.max_depth is None and not unbounded and a.rr_depth is None and a.occlusion is None and not lights and a.env_sampling == "cosine"
        and not a.compact and not a.transmission):
    r = WF.ArrayRenderer(tab, centers, radii, camera=cam, ground_truth=gts, **extra)
else:
    from bsdf_diffusion_sampling_amd.pathtrace import PathArrayRenderer
    r = PathArrayRenderer(tab, centers, radii, camera=cam, ground_truth=gts, **extra,
                          max_depth=None if unbounded else 1 if a.max_depth is None else a.max_depth, rr_depth=a.rr_depth,
                          occlusion=None if a.occlusion is None else bool(a.occlusion), lights=lights, env_sampling=a.env_sampling,
                          env=None if a.no_env or not lights else WF.make_sky(), compact=a.compact, transmission=a.transmission)
r.render(2, a.spp, seed=9); torch.cuda.synchronize()
t0 = time.perf_counter(); img = r.render(a.passes, a.spp, seed=0); torch.cuda.synchronize(); dt = time.perf_counter() - t0
b = r.primary(0, a.height, 1, 0, 0); mat = b["mat"].cpu().numpy(); nb = len(tab)
paths = a.width * a.height * a.spp * a.passes
print(json.dumps({"workload": f"{os.path.splitext(os.path.basename(a.scene))[0] if a.scene else 'array0'}_{a.width}x{a.height}_{a.passes}x{a.spp}spp_{a.domain}", "materials": len(tab),
                  "max_depth": getattr(r, "max_depth", 1), "occlusion": getattr(r, "occlusion", False), "point_lights": len(lights),
                  "env_sampling": a.env_sampling, "rr_depth": getattr(r, "rr_depth", None),
                  "depth": getattr(r, "stats", {}).get("depth"), "depth_cap_hit": getattr(r, "stats", {}).get("depth_cap_hit"),
                  "lanes_per_bounce": getattr(r, "stats", {}).get("lanes_per_bounce"),
                  "compact": getattr(r, "compact", False), "transmission": getattr(r, "transmission", False), "list_per_bounce": getattr(r, "stats", {}).get("list_per_bounce"),
                  "ground_truth_materials": len(gts), "seconds": dt, "passes_per_s": a.passes / dt, "Mpaths_per_s": paths / dt / 1e6,
                  "ball_albedo": "ball_albedo" in extra,
                  "ball_fraction": float((mat < nb).mean()), "floor_fraction": float((mat == nb).mean()), "miss_fraction": float((mat == nb + 1).mean())}))
img = img.cpu().numpy(); os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
np.save(a.out + ".npy", img); write_png(a.out + ".png", tonemap(img))
