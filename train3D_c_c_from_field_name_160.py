"""160^3 conditional VDM training with the learned-linear noise schedule and chs = [48, 96, 192, 384].  Same command line as the
reference script of this name:
    python train3D_c_c_from_field_name_160.py <field_in> <field_out>"""
from vdm4cdm_amd.entry import train3d_c_c

if __name__ == "__main__":
    train3d_c_c("160")
