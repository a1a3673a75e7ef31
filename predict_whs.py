"""The reference's prediction command (predict_whs.py): one uint16 NIfTI label map per "test" image of --json_list under --data_dir, written
to --result_dir (mi-seg_amd/training/predict.py)."""
import __graft_entry__

if __name__ == "__main__":
    __graft_entry__.load_package()
    from mi_seg_amd.training.predict import main
    main()
