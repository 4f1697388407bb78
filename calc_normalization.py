"""Normalisation constants of CAMELS fields from the stacks, on the device (the reference's scripts/calc_normalization.ipynb):

    python calc_normalization.py <field> [<field> ...] [--suite Astrid] [--set LH] [--z z_0.0] [--nside 256] [--alpha A]
                                 [--out normalizations_3d.json]

reads $VDM4CDM_DATA_ROOT/3D_grids_new/Grids_<field>_<suite>_<set>_256_z=....npy (or 3D_grids_<nside>/...), computes the mean and the
population std of log10(field + alpha) in float64 in one streaming pass, and merges {"<field>_m": mean, "<field>_s": std} into --out
(vdm4cdm_amd.data.calc_normalizations).  Point $VDM4CDM_NORMALIZATIONS at that file to train on the field."""
import argparse
import os


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("fields", nargs="+", metavar="field", help="CAMELS field names (Mgas, T, Z, ...)")
    ap.add_argument("--suite", default="Astrid")
    ap.add_argument("--set", dest="set_name", default="LH")
    ap.add_argument("--z", default="z_0.0")
    ap.add_argument("--nside", type=int, default=256, help="grid size of the stack to read (256: 3D_grids_new/)")
    ap.add_argument("--alpha", type=float, default=None, help="alpha of log10(field + alpha); default: the built-in table")
    ap.add_argument("--out", default="normalizations_3d.json", help="JSON file the constants are merged into")
    a = ap.parse_args(argv)
    from vdm4cdm_amd import data
    root = os.environ.get(data.DATA_ROOT_ENV)
    if not root:
        ap.error(f"${data.DATA_ROOT_ENV} is not set: it names the CAMELS directory that holds 3D_grids_new/")
    data.calc_normalizations(root, a.fields, suite=a.suite, set_name=a.set_name, z=a.z, nside=a.nside, alpha=a.alpha, out=a.out)


if __name__ == "__main__":
    main()
