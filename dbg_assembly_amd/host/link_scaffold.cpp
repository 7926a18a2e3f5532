// link_scaffold -- the link_scaffold module's scaffolder (link_scaffold/link_scaffold.cpp + link_func.cpp) with the link table built
// and the scaffold sequences written on the GPU (LINK section of include/dbgk.h).  Same command line, same six output files
// <prefix>.insert<I>.scaffold.{links.all,links.uniq,pos.tab,seq.fa} and .scaffold_repeat.{seq.fa,pos.tab}, same protocol on stderr.
#include "link_common.h"

static int InsertSize = 400;
static int IsMatePair = 0;

static void usage()
{
	cout << "\nFunction instruction:\nlink_scaffold, converts read PEs into contig relations, links the contigs into scaffolds.\
\n(1) If two contigs are neighbor, and they are in the same DNA strand, a pair of PE read will mapped in\
   the F and R way, that is, one read mapped forwardly on one contig, and the other read mapped reversely\
   on the other contig. We use this character to decide the strand relations between two neighbor contigs.\
\n(2) Each contig has two strand forms, we stored both of them in the memory, and each contig node only\
   has one link, the 3'-direction. This can make the strand problem quite easy, and do not increase the\
   memory usage too much.\
\n(3) This program require more than a specified number of read pairs to support two neighbor contigs,\
   and build a graph using neighboring-link-technology, take contig as nodes, and the 3'-link as arcs.\
\n(4) The scaffold sequences were read out from a linear contig, that is, with only one ingoing arc and one\
   outgoing arc, and scaffolding stops at breaking or branching nodes.\n";
	cout << "\nlink_scaffold  <contig_file.fa>  <mapping_twoctg_files.lib>\n"
	     << "   Function: link contigs into scaffolds by pair-end or mate-pair reads, inside gap are not filled" << endl
	     << "   Version: 1.0" << endl
	     << "   -m <int>   input mapping data type: 0, pair-ends; 1. mated-pair,  default=" << IsMatePair << endl
	     << "   -n <int>   the minimum number of read-pairs required to support a link between two contigs, default=" << PairNumCut << endl
	     << "   -i <int>   mean insert size for pair-ends or mated-pair reads, default=" << InsertSize << endl
	     << "   -o <str>   the output file prefix, set in commond-line, default = " << Output_prefix << endl
	     << "   -h         get the help information\n" << endl;
	exit(0);
}

static void output_parameters()
{
	cerr << "link_scaffold  [version 1.0]" << endl
	     << "   -m <int>   input mapping data type: 0, pair-ends; 1. mated-pair,  default=" << IsMatePair << endl
	     << "   -n <int>   the minimum number of read pairs required to support a link between two contigs, default=" << PairNumCut << endl
	     << "   -i <int>   mean insert size for pair-ends or mated-pair reads, default=" << InsertSize << endl
	     << "   -o <str>   the output prefix, set in commond-line, default = " << Output_prefix << endl
	     << "   -h         get the help information\n" << endl;
}

// the fields parse_pair_ends_map_file / parse_mate_pairs_map_file take from one line (link_func.cpp:253-260)
static void parse_map_file(const string &file, dbgk_link *L, size_t n_contigs)
{
	LineReader in(file);
	vector<dbgk_link_pair> batch;
	batch.reserve(BatchRecords);
	auto flush = [&]() {
		const int rc = dbgk_link_add_pairs(L, batch.data(), batch.size());
		if (rc) die("dbgk_link_add_pairs", rc);
		batch.clear();
	};
	string line;
	vector<string> v;
	int id1 = 0, id2 = 0;
	while (in.getline(line)) {
		if (!split_map_line("link_scaffold", file, line, n_contigs, v, id1, id2)) continue;
		dbgk_link_pair r{};
		r.contig1 = id1 / 2; r.start1 = atoi(v[6].c_str()); r.end1 = atoi(v[7].c_str());
		r.contig2 = id2 / 2; r.start2 = atoi(v[16].c_str()); r.end2 = atoi(v[17].c_str());
		r.direct1 = v[8].size() == 1 ? (uint8_t)v[8][0] : (uint8_t)'?';
		r.direct2 = v[18].size() == 1 ? (uint8_t)v[18][0] : (uint8_t)'?';
		batch.push_back(r);
		if (batch.size() >= BatchRecords) flush();
	}
	flush();
}

int main(int argc, char *argv[])
{
	int c;
	while ((c = getopt(argc, argv, "m:n:i:o:h")) != -1) {
		switch (c) {
			case 'm': IsMatePair = atoi(optarg); break;
			case 'n': PairNumCut = atoi(optarg); break;
			case 'i': InsertSize = atoi(optarg); break;
			case 'o': Output_prefix = optarg; break;
			case 'h': usage(); break;
			default: usage();
		}
	}
	if (argc < 3 || argc - optind < 2) usage();
	output_parameters();
	const string contig_seq_file = argv[optind++];
	const string para_map_file = argv[optind++];

	const clock_t time_start = clock();
	auto run_time = [&]() { cerr << "Run time: " << double(clock() - time_start) / CLOCKS_PER_SEC << endl; };
	cerr << "\nProgram start ............" << endl;
	run_time();

	vector<string> contig_ids, contig_seqs;
	vector<uint32_t> lens;
	uint64_t contig_total_len = 0;
	load_contigs("link_scaffold", contig_seq_file, contig_ids, contig_seqs, lens, contig_total_len);
	const size_t n_contigs = contig_seqs.size();

	vector<string> Paired_map_files;
	reading_lib_file(para_map_file, Paired_map_files);
	cerr << "\nInput reads mapping files number: " << Paired_map_files.size() << endl;
	run_time();

	if (IsMatePair != 0 && IsMatePair != 1) { // the reference parses nothing then
		cerr << "link_scaffold: -m must be 0 or 1" << endl;
		return 1;
	}
	dbgk_link *L = nullptr;
	dbgk_link_params P{IsMatePair, PairNumCut, InsertSize};
	int rc = dbgk_link_create(&P, 0, &L);
	if (rc) die("dbgk_link_create", rc);
	if ((rc = dbgk_link_set_contigs(L, lens.data(), n_contigs))) die("dbgk_link_set_contigs", rc);
	for (size_t i = 0; i < Paired_map_files.size(); i++) {
		cerr << "\nparse map file: " << Paired_map_files[i] << endl;
		parse_map_file(Paired_map_files[i], L, n_contigs);
	}
	if ((rc = dbgk_link_build(L))) die("dbgk_link_build", rc);
	cerr << "\nParsed the map files done !" << endl;
	run_time();

	const size_t n_nodes = 2 * n_contigs + 1;
	vector<uint64_t> first(n_nodes + 1);
	uint64_t n_links = 0;
	dbgk_link_counters ctr{};
	if ((rc = dbgk_link_export(L, first.data(), nullptr, 0, &n_links, &ctr))) die("dbgk_link_export", rc);
	report_link_classes(ctr);

	dbgk_link_summary S{};
	if ((rc = dbgk_link_resolve(L, &S))) die("dbgk_link_resolve", rc);
	cerr << "\nRemoved LowFreq link num: " << S.lowfreq << endl;
	auto snapshot = [&](int stage, uint8_t *inlink, uint8_t *link, dbgk_link_entry *e) {
		if (int rc = dbgk_link_snapshot(L, stage, inlink, link, e)) die("dbgk_link_snapshot", rc);
	};
	report_3prime_links(snapshot, n_nodes);
	const string stem = Output_prefix + ".insert" + to_string(InsertSize);
	display_data_in_link(snapshot, 0, first, stem + ".scaffold.links.all");
	cerr << "\nRemoved interleave links num: " << S.interleave << endl;
	cerr << "\nRemoved repeat nodes num: " << S.repeat_nodes << endl;
	cerr << "\nRemoved links [related with repeat or small nodes] num: " << S.deleted << endl;
	display_data_in_link(snapshot, 1, first, stem + ".scaffold.links.uniq");

	// read_out_scaffold (link_scaffold.cpp:300-423): the layout comes sorted, the sequences of all scaffolds from one device call
	vector<uint64_t> scaf_first(S.scaffolds + 1);
	vector<dbgk_link_item> items(S.items + 1);
	vector<int32_t> repeats(S.repeat_nodes + 1);
	if ((rc = dbgk_link_layout(L, scaf_first.data(), items.data(), repeats.data()))) die("dbgk_link_layout", rc);
	string bases;
	vector<uint64_t> offsets;
	concat(contig_seqs, bases, offsets);
	const string seq = emit_sequences([&](char *out, uint64_t capacity, uint64_t *out_len) {
		return dbgk_link_emit(L, bases.data(), offsets.data(), n_contigs, items.data(), S.items, out, capacity, out_len);
	}, "dbgk_link_emit");

	ofstream ScafPosFile((stem + ".scaffold.pos.tab").c_str());
	if (!ScafPosFile) cerr << "fail to open file" << stem + ".scaffold.pos.tab" << endl;
	ofstream ScafSeqFile((stem + ".scaffold.seq.fa").c_str());
	if (!ScafSeqFile) cerr << "fail to open file" << stem + ".scaffold.seq.fa" << endl;
	uint64_t total_scaffold_len = 0, total_scaffold_lenwogap = 0;
	ContigTally included;
	int scaffold_id = -1;
	uint64_t seq_pos = 0;
	for (uint64_t s = 0; s < S.scaffolds; s++) {
		scaffold_id += 2;
		int scaf_ctg_num = 0, scaf_len = 0, scaf_lenwogap = 0;
		string pos;
		for (uint64_t t = scaf_first[s]; t < scaf_first[s + 1]; t++) {
			const dbgk_link_item &it = items[t];
			const int block_start = scaf_len + 1;
			if (it.contig >= 0) {
				const int block_size = (int)lens[it.contig];
				scaf_ctg_num++;
				scaf_len += block_size;
				scaf_lenwogap += block_size;
				pos += "\t" + contig_ids[it.contig] + "\t" + to_string(block_start) + "\t" + to_string(scaf_len) + "\t" + to_string(block_size) + "\t" +
				       (it.value ? "R" : "F") + "\n";
				included.num++;
				included.len += block_size;
			} else {
				scaf_len += it.value;
				pos += "\tgap\t" + to_string(block_start) + "\t" + to_string(scaf_len) + "\t" + to_string(it.value) + "\tN\n";
			}
		}
		ScafSeqFile << ">scf_" << scaffold_id << "   fragment_num:" << scaf_ctg_num << "   length:" << scaf_len << "   lenwogap:" << scaf_lenwogap << "\n";
		ScafSeqFile.write(seq.data() + seq_pos, scaf_len);
		ScafSeqFile << "\n";
		seq_pos += (uint64_t)scaf_len;
		ScafPosFile << ">scf_" << scaffold_id << "\n" << pos;
		total_scaffold_len += scaf_len;
		total_scaffold_lenwogap += scaf_lenwogap;
	}
	ScafPosFile.close();
	ScafSeqFile.close();

	const ContigTally excluded =
	    write_repeat_contigs(stem + ".scaffold_repeat", "scf_", scaffold_id, repeats, S.repeat_nodes, contig_ids, contig_seqs, lens);

	cerr << "\nRead out scaffold sequence done" << endl;
	cerr << "\nTotal scaffold number:          " << S.scaffolds << endl;
	cerr << "Total scaffold length[WithGap]: " << total_scaffold_len << endl;
	cerr << "Total scaffold length[NoGap]:   " << total_scaffold_lenwogap << endl;
	report_contig_use(included, excluded, n_contigs, contig_total_len);
	cerr << "\nProgram finished !" << endl;
	run_time();
	dbgk_link_destroy(L);
	return 0;
}
