"""Down-gridded CAMELS training sets from the 256^3 cubes, on the device (the reference's scripts/make_down_grids.ipynb):

    python make_down_grids.py <nside> [--fields Mcdm Mstar] [--sets LH CV 1P] [--suite Astrid] [--z z_0.0] [--overwrite]

reads $VDM4CDM_DATA_ROOT/3D_grids_new/Grids_<field>_<suite>_<set>_256_z=....npy and writes
$VDM4CDM_DATA_ROOT/3D_grids_<nside>/Grids_<field>_<suite>_<set>_<nside>_z=....npy (vdm4cdm_amd.data.make_down_grids)."""
import argparse
import os


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("nside", type=int, help="edge of the down-gridded cubes (128, 160, 176, 192, 224)")
    ap.add_argument("--fields", nargs="+", default=["Mcdm", "Mstar"])
    ap.add_argument("--sets", nargs="+", default=["LH", "CV", "1P"])
    ap.add_argument("--suite", default="Astrid")
    ap.add_argument("--z", default="z_0.0")
    ap.add_argument("--overwrite", action="store_true", help="rewrite targets that already exist")
    a = ap.parse_args(argv)
    from vdm4cdm_amd import data
    root = os.environ.get(data.DATA_ROOT_ENV)
    if not root:
        ap.error(f"${data.DATA_ROOT_ENV} is not set: it names the CAMELS directory that holds 3D_grids_new/")
    data.make_down_grids(root, a.nside, fields=a.fields, sets=a.sets, suite=a.suite, z=a.z, overwrite=a.overwrite)


if __name__ == "__main__":
    main()
