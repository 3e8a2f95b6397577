// nh_taxa.h -- the taxa manifest of nh_build_db (nh_build_args.taxa_file): host only, no device, no HIP.
//
//   taxid <TAB> parent taxid <TAB> name [<TAB> FASTA path]...
//
// one taxon a line; `#` lines and empty lines are skipped, CRLF is tolerated.  A line without a path is an inner node; a node with
// children may carry sequences too.  Parent 1 is the root, which is implicit and never a line.  Relative paths resolve against the
// manifest's directory.  Internal ids: 0 the null sentinel, 1 the root, then breadth first with the children of a node in ascending
// external id -- parents lie below their children, and the lowest common ancestor of two nodes is found by walking the larger id up.
#ifndef NH_TAXA_H
#define NH_TAXA_H
#include <stdint.h>

#include <string>
#include <vector>

namespace nh {

constexpr uint32_t TAXA_MAX_NODES = 4096;  // taxa and the root; with the sentinel 4097 values: value_bits <= 13

struct TaxaNode {
    uint64_t taxid = 0;              // external id
    uint32_t parent = 0;             // internal id of the parent (0 for the sentinel and the root)
    uint32_t first_child = 0, children = 0;
    uint32_t line = 0;               // of the manifest (0: the sentinel, the root)
    std::string name;
    std::string rank = "no rank";    // (a manifest knows no rank: only a node taken over from a base database has another)
    std::vector<std::string> files;  // FASTA paths, resolved
};

// the taxonomy of a database that is being extended (taxo.k2d), by internal id
struct BaseTaxo {
    std::vector<uint32_t> parent;
    std::vector<uint64_t> taxid;
    std::vector<std::string> name, rank;
};

// the manifest at `path` -> nodes in internal-id order ([0] the sentinel, [1] the root).  NH_OK, or NH_EINVAL / NH_EIO with a
// message that names the file and the line.
int parse_taxa(const char *path, std::vector<TaxaNode> &nodes, std::string &err);

// taxo.k2d at `path` -> t.  NH_OK; NH_EIO; NH_EDB for a bad magic, a truncated file, a parent that does not lie below its child, a
// root whose external id is not 1 or an external id that two nodes share; NH_EINVAL for more than TAXA_MAX_NODES nodes.
int read_base_taxo(const char *path, BaseTaxo &t, std::string &err);

// The manifest at `path` on top of `base` (nh_extend_db): a line's parent may be 1, another line or an external id of the base; a
// line whose taxid the base holds adds its files to that node, must name the base's parent, and the base's name and rank stay.
// The merged tree is numbered like any other, so remap[internal id of the base] is the node's internal id in `nodes`.  What
// parse_taxa refuses is refused here; NH_EINVAL too for an existing taxid under another parent and for more than TAXA_MAX_NODES
// merged nodes.
int merge_taxa(const char *path, const BaseTaxo &base, std::vector<TaxaNode> &nodes, std::vector<uint32_t> &remap, std::string &err);
// the same for one taxon without a manifest: a child of the root, or the base's node of that taxid
int merge_taxon(uint64_t taxid, const std::string &name, const std::vector<std::string> &files, const BaseTaxo &base, std::vector<TaxaNode> &nodes,
                std::vector<uint32_t> &remap, std::string &err);

// bits of a cell's value field for that many nodes, the sentinel included (2 for three nodes)
inline uint32_t value_bits_for(uint32_t node_count) {
    uint32_t b = 1;
    while ((1u << b) < node_count) b++;
    return b;
}

}  // namespace nh
#endif
